"""GPU: a plan's grow-only buffers on a live context. One plan runs rescale, rotate, rns_ntt_fwd / rns_ntt_inv, multiply_plain, ct_lincomb,
ckks_encode / ckks_decode, sample (a small kind) and rlwe_encrypt on a batch of 3 and is closed; a fresh plan on the SAME context runs
the same calls on a batch of 5 whose first three instances are the same inputs, so every scratch buffer and every allocate-once table
of the plan is allocated again, larger, while the context lives on. Every word of the first three instances must be what the first plan
wrote. n = 1024, L = 2, K = 3."""
import numpy as np
import pytest

from ks_util import KsCase

pytestmark = pytest.mark.gpu

N, L, K = 1024, 2, 3
SEED = bytes(range(32))
SCALE = float(1 << 30)


def run_all(hx, ctx, dev, orc, case, batch):
    """every call on a fresh plan; {name: (device tensor, words per instance)}"""
    import torch
    plan = hx.KeySwitchPlan(ctx, N, L, K, L + 1, 2, case.moduli, case.modswitch)
    plan.set_keys(case.keys)
    qs = [int(q) for q in case.moduli]

    def words(limbs, comps, salt):                                 # [batch][comps][limbs][N] below the limb's modulus, instance b the same in every batch
        a = np.stack([np.concatenate([orc.splitmix(N, salt + 1000 * b + 10 * k + i, qs[i]) for k in range(comps) for i in range(limbs)])
                      for b in range(batch)])
        return hx.as_i64(a.reshape(-1)).to(dev)

    def blank(count, dtype=torch.int64):
        return torch.full((count,), -1, dtype=torch.int64, device=dev).view(dtype)

    out = {}
    ct, ct3 = words(L, 2, 1), words(K, 1, 2)
    pt, other = words(L, 1, 3), words(L, 2, 4)

    out["rescale"] = blank(batch * 2 * (L - 1) * N)
    plan.rescale(out["rescale"], ct, batch, L, 2)
    out["rotate"] = blank(batch * 2 * L * N)
    plan.rotate(out["rotate"], ct, batch, 5)
    out["rns_ntt_fwd"] = blank(batch * K * N)
    plan.rns_ntt_fwd(out["rns_ntt_fwd"], ct3, batch, K)
    out["rns_ntt_inv"] = blank(batch * K * N)
    plan.rns_ntt_inv(out["rns_ntt_inv"], ct3, batch, K)
    out["multiply_plain"] = blank(batch * 2 * L * N)
    plan.multiply_plain(out["multiply_plain"], ct, pt, batch, 2, L, batch)
    out["ct_lincomb"] = blank(batch * 2 * L * N)
    plan.ct_lincomb(out["ct_lincomb"], [ct, other], batch, 2, L, weights=[[3, qs[1] - 1], [qs[0] - 2, 7]], pt=pt, pt_batch=batch,
                    const=[5, 6])
    slots = np.stack([np.sin(np.arange(N, dtype=np.float64) * (b + 1) * 0.37) for b in range(batch)])     # [batch][N/2][2]
    out["ckks_encode"] = blank(batch * L * N)
    plan.ckks_encode(out["ckks_encode"], torch.from_numpy(slots.reshape(-1)).to(dev), batch, L, SCALE)
    out["ckks_decode"] = blank(batch * N, torch.float64)
    plan.ckks_decode(out["ckks_decode"], out["ckks_encode"], batch, L, SCALE)
    out["sample"] = blank(batch * L * N)
    plan.sample(out["sample"], hx.SAMPLE_TERNARY, batch, L, seed=SEED, stream=3, first=7)
    secret = blank(L * N)
    plan.sample(secret, hx.SAMPLE_TERNARY, 1, L, seed=SEED, stream=77, first=0)
    out["rlwe_encrypt"] = blank(batch * 2 * L * N)
    plan.rlwe_encrypt(out["rlwe_encrypt"], secret, batch, L, pt=pt, pt_batch=batch, seed=SEED, stream=4, first=11)
    ctx.sync()
    assert plan.range_check(), "every input word is below its modulus"
    plan.close()
    return {name: (t, t.numel() // batch) for name, t in out.items()}


def test_fresh_plan_regrows_every_buffer_on_a_live_context(hx, ctx, dev, orc):
    import torch
    case = KsCase(orc, N, L, K, seed=5)
    first = run_all(hx, ctx, dev, orc, case, 3)
    kept = {name: t.clone() for name, (t, _) in first.items()}
    second = run_all(hx, ctx, dev, orc, case, 5)
    for name, (t, per) in second.items():
        got, want = t[:3 * per].view(torch.int64), kept[name].view(torch.int64)
        assert got.numel() == want.numel() == 3 * per
        if not torch.equal(got, want):
            at = int((got != want).nonzero()[0])
            pytest.fail(f"{name}: word {at % per} of instance {at // per} differs between the plan of batch 3 and the fresh plan of batch 5")
        assert bool((t[3 * per:].view(torch.int64) != -1).any()), f"{name}: instances 3 and 4 were not written"
