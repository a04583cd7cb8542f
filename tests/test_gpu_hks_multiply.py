"""GPU: the hybrid multiply (hexl_hks_multiply_sum_relinearize, hexl_hks_relinearize_rescale, hexl_hks_multiply_sum_rescale) word for
word against tests/hks_mul_model.py: a ragged last digit and the smallest rescaling level (L = 3, K = 5, alpha = 2, levels 3 and 2), one
limb per digit (alpha = 1), one digit at every level (alpha = 3 = L), test_gpu_hks.py's mixed-tier chain, extreme operands; one and three
terms with a square and an operand read through more limbs than the level; the word identities with hexl_ct_tensor_sum followed by
hexl_hks_relinearize / hexl_hks_relinearize_rescale on the device; n = 16384 and n = 32768; two scratch chunks (a child process with
HEXL_KS_CHUNK) and a regrow followed by a smaller call; a non-blocking caller stream; every rejection; and end to end: encode ->
encrypt -> multiply_sum_rescale with a key from gen_hybrid_key -> decrypt -> decode within the noise bound of the definition."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from ckks_model import Limbs
from hks_mul_model import HksMul
from ks_util import KsCase, seal_chain
from rns_model import assert_instances
from test_gpu_hks import Setup, minus_one, torch_, up

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("component", "limb", "coefficient")
HEXL_E_BADARG, HEXL_E_NOKEYS = -1, -2


def mul_model(orc, s):
    return HksMul(orc, s.n, s.L, s.K, s.alpha, s.qs)


def terms(s, l, n_terms, distinct):
    """per instance b < distinct: (a_s, b_s) of a sum of n_terms products at level l, and in_limbs. Three terms: a plain pair, a square
    (the same array twice) and a pair whose first operand has K limbs and is read through its first l."""
    il = None if n_terms == 1 else [[l, l], [l, l], [s.K, l]]
    per = []
    for b in range(distinct):
        a0, b0 = s.words(2, l, b, 11), s.words(2, l, b, 12)
        if n_terms == 1:
            per.append(([a0], [b0]))
        else:
            sq, wide, b2 = s.words(2, l, b, 13), s.words(2, s.K, b, 14), s.words(2, l, b, 15)
            per.append(([a0, sq, wide], [b0, sq, b2]))
    return per, il


def device_terms(hx, dev, per, batch):
    """the operand lists on the device, stacked over the batch (instance b = per[b % distinct]); a square is ONE tensor given twice"""
    n_terms, distinct = len(per[0][0]), len(per)
    d_as = [up(hx, dev, np.stack([per[b % distinct][0][t] for b in range(batch)])) for t in range(n_terms)]
    d_bs = [d_as[t] if per[0][1][t] is per[0][0][t] else up(hx, dev, np.stack([per[b % distinct][1][t] for b in range(batch)]))
            for t in range(n_terms)]
    return d_as, d_bs


def run_level(hx, ctx, dev, s, hm, keys, l, batch, label, distinct=2):
    """relinearize_rescale and multiply_sum_rescale (one and three terms) at level l against the model, every word of every instance"""
    n = s.n
    ct3 = [s.words(3, l, b, 4) for b in range(distinct)]
    d_ct3 = up(hx, dev, np.stack([ct3[b % distinct] for b in range(batch)]))
    out = minus_one(dev, batch * 2 * (l - 1) * n)
    s.hks.relinearize_rescale(out, d_ct3, batch, l)
    ctx.sync()
    assert_instances(hx.to_u64(out), [hm.relinearize_rescale(keys, c, l) for c in ct3], batch, NAMES, (2, l - 1, n), f"{label}: relinearize_rescale level {l}")
    assert np.array_equal(hx.to_u64(d_ct3), np.stack([ct3[b % distinct] for b in range(batch)]).reshape(-1)), "the input was written"
    for n_terms in (1, 3):
        per, il = terms(s, l, n_terms, distinct)
        d_as, d_bs = device_terms(hx, dev, per, batch)
        out = minus_one(dev, batch * 2 * (l - 1) * n)
        s.hks.multiply_sum_rescale(out, d_as, d_bs, batch, l, in_limbs=il)
        ctx.sync()
        want = [hm.multiply_sum_rescale(keys, a, b, l, il) for a, b in per]
        assert_instances(hx.to_u64(out), want, batch, NAMES, (2, l - 1, n), f"{label}: multiply_sum_rescale level {l}, {n_terms} term(s)")


SHAPES = {
    # name: (L, alpha, K, moduli, family, levels, batch)
    "a2_ragged": (3, 2, 5, lambda orc, n: orc.primes(5, 51, n), "uniform", (3, 2), 3),
    "a2_extreme": (3, 2, 5, lambda orc, n: orc.primes(5, 51, n), "extreme", (3, 2), 3),
    "a1_per_limb_digits": (3, 1, 5, lambda orc, n: orc.primes(5, 51, n), "uniform", (3, 2), 3),
    "a3_one_digit": (3, 3, 5, lambda orc, n: orc.primes(5, 50, n), "uniform", (3, 2), 3),
    "mixed_tier": (4, 2, 6, lambda orc, n: seal_chain(orc, 6, n), "extreme", (4, 2), 2),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rescaling_calls_match_the_model(hx, ctx, dev, orc, shape):
    L, alpha, K, mod, family, levels, batch = SHAPES[shape]
    s = Setup(hx, ctx, orc, 1024, L, K, alpha, mod(orc, 1024), family)
    if shape == "mixed_tier":
        tiers, mixed = s.plan.tiers()
        assert mixed and tiers[0] == 0 and all(t != 0 for t in tiers[1:]), tiers
    hm = mul_model(orc, s)
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    for l in levels:
        run_level(hx, ctx, dev, s, hm, keys, l, batch, shape)
    assert s.hks.mul_scratch_bytes(1) == s.hks.scratch_bytes(1) + 3 * L * 1024 * 8
    s.close()


@pytest.mark.parametrize("l", [2, 3])
def test_word_identities_on_the_device(hx, ctx, dev, orc, l):
    """multiply_sum_relinearize = ct_tensor_sum -> hks relinearize; multiply_sum_rescale = ct_tensor_sum -> relinearize_rescale"""
    torch = torch_()
    n, L, K, batch = 1024, 3, 5, 3
    s = Setup(hx, ctx, orc, n, L, K, 2, orc.primes(K, 51, n))
    hm = mul_model(orc, s)
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    per, il = terms(s, l, 3, batch)
    d_as, d_bs = device_terms(hx, dev, per, batch)
    ct3 = minus_one(dev, batch * 3 * l * n)
    s.plan.ct_tensor_sum(ct3, d_as, d_bs, batch, l, in_limbs=il)
    two, fused = minus_one(dev, batch * 2 * l * n), minus_one(dev, batch * 2 * l * n)
    s.hks.relinearize(two, ct3, batch, l)
    s.hks.multiply_sum_relinearize(fused, d_as, d_bs, batch, l, in_limbs=il)
    two_rs, fused_rs = minus_one(dev, batch * 2 * (l - 1) * n), minus_one(dev, batch * 2 * (l - 1) * n)
    s.hks.relinearize_rescale(two_rs, ct3, batch, l)
    s.hks.multiply_sum_rescale(fused_rs, d_as, d_bs, batch, l, in_limbs=il)
    ctx.sync()
    assert torch.equal(fused, two), "multiply_sum_relinearize is not ct_tensor_sum followed by relinearize"
    assert torch.equal(fused_rs, two_rs), "multiply_sum_rescale is not ct_tensor_sum followed by relinearize_rescale"
    want = [hm.multiply_sum_relinearize(keys, a, b, l, il) for a, b in per]
    assert_instances(hx.to_u64(fused), want, batch, NAMES, (2, l, n), f"multiply_sum_relinearize level {l}")
    s.close()


def test_plain_and_rescaling_mod_downs_alternate_on_one_object(hx, ctx, dev, orc):
    """The two mod-downs share their constants tables and their stage function. One object, calls back to back without recreating it:
    keyswitch l = 3, relinearize_rescale l = 3, keyswitch l = 3, relinearize_rescale l = 2 (the smallest level with a rescaling row),
    relinearize l = 1 (row 0 of the mod-up beside row 0 of the divisor table), relinearize_rescale l = 3. Every output word against the
    models, and the repeated calls bit-equal to their first occurrence: a row mix-up, or a row pointer left over from the call before."""
    torch = torch_()
    n, L, K, batch = 1024, 3, 5, 3
    s = Setup(hx, ctx, orc, n, L, K, 2, orc.primes(K, 51, n))
    hm = mul_model(orc, s)
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    ts, rs = [s.words(1, 3, b, 1) for b in range(batch)], [s.words(2, 3, b, 2) for b in range(batch)]
    ct3 = {l: [s.words(3, l, b, 4) for b in range(batch)] for l in (1, 2, 3)}
    d_t = up(hx, dev, np.stack(ts))
    d_ct3 = {l: up(hx, dev, np.stack(ct3[l])) for l in ct3}

    def keyswitch():
        d_r = up(hx, dev, np.stack(rs))
        s.hks.keyswitch(d_r, d_t, batch, 3)
        return d_r

    def rescale(l):
        out = minus_one(dev, batch * 2 * (l - 1) * n)
        s.hks.relinearize_rescale(out, d_ct3[l], batch, l)
        return out

    ks_a, rs3_a, ks_b, rs2 = keyswitch(), rescale(3), keyswitch(), rescale(2)
    relin1 = minus_one(dev, batch * 2 * 1 * n)
    s.hks.relinearize(relin1, d_ct3[1], batch, 1)
    rs3_b = rescale(3)
    ctx.sync()
    assert_instances(hx.to_u64(ks_a), [s.model.keyswitch(keys, ts[b], rs[b], 3) for b in range(batch)], batch, NAMES, (2, 3, n), "keyswitch level 3")
    assert_instances(hx.to_u64(rs3_a), [hm.relinearize_rescale(keys, c, 3) for c in ct3[3]], batch, NAMES, (2, 2, n), "relinearize_rescale level 3")
    assert_instances(hx.to_u64(rs2), [hm.relinearize_rescale(keys, c, 2) for c in ct3[2]], batch, NAMES, (2, 1, n), "relinearize_rescale level 2")
    assert_instances(hx.to_u64(relin1), [s.model.relinearize(keys, c, 1) for c in ct3[1]], batch, NAMES, (2, 1, n), "relinearize level 1")
    assert torch.equal(ks_b, ks_a), "the second keyswitch at level 3 differs from the first"
    assert torch.equal(rs3_b, rs3_a), "the second relinearize_rescale at level 3 differs from the first"
    s.close()


def test_multiply_sum_relinearize_takes_level_one(hx, ctx, dev, orc):
    n, L, K = 1024, 3, 5
    s = Setup(hx, ctx, orc, n, L, K, 2, orc.primes(K, 51, n))
    hm = mul_model(orc, s)
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    per, il = terms(s, 1, 1, 2)
    d_as, d_bs = device_terms(hx, dev, per, 2)
    out = minus_one(dev, 2 * 2 * n)
    s.hks.multiply_sum_relinearize(out, d_as, d_bs, 2, 1)
    ctx.sync()
    assert_instances(hx.to_u64(out), [hm.multiply_sum_relinearize(keys, a, b, 1) for a, b in per], 2, NAMES, (2, 1, n), "level 1")
    s.close()


@pytest.mark.parametrize("n", [16384, 32768])
def test_large_rings(hx, ctx, dev, orc, n):
    """the other register geometries of the workgroup kernels and the grouped epilogue: L = 2, K = 3, alpha = 1, level 2, batch 1"""
    s = Setup(hx, ctx, orc, n, 2, 3, 1, orc.primes(3, 51, n))
    hm = mul_model(orc, s)
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    ct3 = s.words(3, 2, 0, 4)
    out = minus_one(dev, 2 * n)
    s.hks.relinearize_rescale(out, up(hx, dev, ct3), 1, 2)
    per, _ = terms(s, 2, 1, 1)
    d_as, d_bs = device_terms(hx, dev, per, 1)
    out2 = minus_one(dev, 2 * n)
    s.hks.multiply_sum_rescale(out2, d_as, d_bs, 1, 2)
    ctx.sync()
    assert_instances(hx.to_u64(out), [hm.relinearize_rescale(keys, ct3, 2)], 1, NAMES, (2, 1, n), f"relinearize_rescale n = {n}")
    assert_instances(hx.to_u64(out2), [hm.multiply_sum_rescale(keys, per[0][0], per[0][1], 2)], 1, NAMES, (2, 1, n), f"multiply_sum_rescale n = {n}")
    s.close()


CHUNK_CASE = dict(n=1024, L=3, K=5, alpha=2, distinct=3, batches=(2, 5, 3))


def chunk_calls(hx, ctx, dev, orc):
    """the three calls at batch 2, then 5 (a regrow), then 3 on ONE object, over three distinct instances -> {name: words}; the parent
    (one chunk per call) and the child (HEXL_KS_CHUNK=2: batch 5 is two chunks and a tail of one) run the same calls"""
    c = CHUNK_CASE
    s = Setup(hx, ctx, orc, c["n"], c["L"], c["K"], c["alpha"], orc.primes(c["K"], 51, c["n"]))
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    L, n = c["L"], c["n"]
    ct3 = [s.words(3, L, b, 4) for b in range(c["distinct"])]
    per, il = terms(s, L, 3, c["distinct"])
    res = {}
    for nb in c["batches"]:
        d_ct3 = up(hx, dev, np.stack([ct3[b % c["distinct"]] for b in range(nb)]))
        d_as, d_bs = device_terms(hx, dev, per, nb)
        rr, mrs, mr = minus_one(dev, nb * 2 * (L - 1) * n), minus_one(dev, nb * 2 * (L - 1) * n), minus_one(dev, nb * 2 * L * n)
        s.hks.relinearize_rescale(rr, d_ct3, nb, L)
        s.hks.multiply_sum_rescale(mrs, d_as, d_bs, nb, L, in_limbs=il)
        s.hks.multiply_sum_relinearize(mr, d_as, d_bs, nb, L, in_limbs=il)
        ctx.sync()
        res.update({f"rr{nb}": hx.to_u64(rr), f"mrs{nb}": hx.to_u64(mrs), f"mr{nb}": hx.to_u64(mr)})
    return s, keys, ct3, per, il, res


def test_two_scratch_chunks_and_a_regrow(hx, ctx, dev, orc, tmp_path):
    c = CHUNK_CASE
    s, keys, ct3, per, il, res = chunk_calls(hx, ctx, dev, orc)
    assert s.hks.mul_scratch_bytes(2) < s.hks.mul_scratch_bytes(5), "this process must run batch 5 in one chunk"
    hm = mul_model(orc, s)
    L, n = c["L"], c["n"]
    want_rr = [hm.relinearize_rescale(keys, x, L) for x in ct3]
    want_mrs = [hm.multiply_sum_rescale(keys, a, b, L, il) for a, b in per]
    want_mr = [hm.multiply_sum_relinearize(keys, a, b, L, il) for a, b in per]
    for nb in c["batches"]:                                       # instance b of every call holds the words of distinct instance b % 3
        assert_instances(res[f"rr{nb}"], want_rr, nb, NAMES, (2, L - 1, n), f"relinearize_rescale batch {nb}")
        assert_instances(res[f"mrs{nb}"], want_mrs, nb, NAMES, (2, L - 1, n), f"multiply_sum_rescale batch {nb}")
        assert_instances(res[f"mr{nb}"], want_mr, nb, NAMES, (2, L, n), f"multiply_sum_relinearize batch {nb}")
    s.close()
    ref = tmp_path / "one_chunk.npz"
    np.savez(ref, **res)
    code = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch, hexl_fpga_amd as hx, orc
from test_gpu_hks_multiply import chunk_calls
dev = torch.device("cuda:0")
ctx = hx.Context(0)
s, keys, ct3, per, il, res = chunk_calls(hx, ctx, dev, orc)
assert s.hks.mul_scratch_bytes(2) == s.hks.mul_scratch_bytes(100) > s.hks.mul_scratch_bytes(1), "HEXL_KS_CHUNK=2 not in force"
want = np.load(%r)
for name in want.files:
    assert np.array_equal(res[name], want[name]), name + " differs from the one-chunk words"
s.close()
print("CHUNKS OK")
''' % (str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests"), str(ref))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, HEXL_KS_CHUNK="2"))
    print(out.stdout[-1000:], out.stderr[-1500:])
    assert out.returncode == 0 and "CHUNKS OK" in out.stdout


def test_on_a_non_blocking_caller_stream(hx, dev, orc):
    torch = torch_()
    own = hx.Context(0, use_torch_stream=False)
    side = torch.cuda.Stream()
    own.set_stream(side.cuda_stream)
    n, l = 1024, 3
    s = Setup(hx, own, orc, n, 3, 5, 2, orc.primes(5, 51, n))
    hm = mul_model(orc, s)
    keys = s.keys()
    d_keys = up(hx, dev, keys)
    per, _ = terms(s, l, 1, 2)
    d_as, d_bs = device_terms(hx, dev, per, 2)
    out = minus_one(dev, 2 * 2 * (l - 1) * n)
    torch.cuda.synchronize()                                      # the uploads ran on torch's stream
    s.hks.set_keys_device(d_keys)
    s.hks.multiply_sum_rescale(out, d_as, d_bs, 2, l)
    side.synchronize()
    assert_instances(hx.to_u64(out), [hm.multiply_sum_rescale(keys, a, b, l) for a, b in per], 2, NAMES, (2, l - 1, n), "side stream")
    own.use_own_stream()
    s.close()
    own.close()


def test_every_rejection(hx, ctx, dev, orc):
    torch = torch_()
    n, L, K = 1024, 3, 5
    s = Setup(hx, ctx, orc, n, L, K, 2, orc.primes(K, 51, n))
    lib = hx.lib()
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    a = torch.zeros(2 * 2 * K * n, dtype=torch.int64, device=dev)           # an operand of up to K limbs, batch 2
    b = torch.zeros(2 * 2 * K * n, dtype=torch.int64, device=dev)
    ct3 = torch.zeros(2 * 3 * L * n, dtype=torch.int64, device=dev)
    out = minus_one(dev, 2 * 2 * L * n)
    h, p = s.hks.h, lambda x: vp(x.data_ptr())
    ops_a, ops_b = (vp * 2)(a.data_ptr(), a.data_ptr()), (vp * 2)(b.data_ptr(), a.data_ptr())
    with_null = (vp * 2)(a.data_ptr(), None)
    limbs = lambda *v: (u64 * len(v))(*v)
    fused = (lib.hexl_hks_multiply_sum_relinearize, lib.hexl_hks_multiply_sum_rescale)
    for batch in (2, 0):
        # before an install: malformed arguments first, then HEXL_E_NOKEYS
        for fn in fused:
            assert fn(h, p(out), ops_a, ops_b, None, 2, batch, L) == HEXL_E_NOKEYS
            assert fn(None, p(out), ops_a, ops_b, None, 2, batch, L) == HEXL_E_BADARG
            assert fn(h, None, ops_a, ops_b, None, 2, batch, L) == HEXL_E_BADARG
            assert fn(h, p(out), None, ops_b, None, 2, batch, L) == HEXL_E_BADARG
            assert fn(h, p(out), ops_a, None, None, 2, batch, L) == HEXL_E_BADARG
            assert fn(h, p(out), with_null, ops_b, None, 2, batch, L) == HEXL_E_BADARG        # a null array entry
            assert fn(h, p(out), ops_a, with_null, None, 2, batch, L) == HEXL_E_BADARG
            for n_terms in (0, 9):
                assert fn(h, p(out), ops_a, ops_b, None, n_terms, batch, L) == HEXL_E_BADARG
            for l in (0, L + 1):
                assert fn(h, p(out), ops_a, ops_b, None, 2, batch, l) == HEXL_E_BADARG
            assert fn(h, p(out), ops_a, ops_b, limbs(L, L, L - 1, L), 2, batch, L) == HEXL_E_BADARG      # in_limbs below the level
            assert fn(h, p(out), ops_a, ops_b, limbs(L, K + 1, L, L), 2, batch, L) == HEXL_E_BADARG      # ... above K
            assert fn(h, p(out), ops_a, ops_b, limbs(L, K, K, L), 2, batch, L) == HEXL_E_NOKEYS          # ... inside l ... K
            assert fn(h, p(out), ops_a, ops_b, None, 2, 1 << 62, L) == HEXL_E_BADARG                     # a size that overflows
        assert lib.hexl_hks_relinearize_rescale(h, p(out), p(ct3), batch, L) == HEXL_E_NOKEYS
        assert lib.hexl_hks_relinearize_rescale(None, p(out), p(ct3), batch, L) == HEXL_E_BADARG
        assert lib.hexl_hks_relinearize_rescale(h, None, p(ct3), batch, L) == HEXL_E_BADARG
        assert lib.hexl_hks_relinearize_rescale(h, p(out), None, batch, L) == HEXL_E_BADARG
        for l in (0, 1, L + 1):                                   # level 1 has nothing to rescale to
            assert lib.hexl_hks_relinearize_rescale(h, p(out), p(ct3), batch, l) == HEXL_E_BADARG
        assert lib.hexl_hks_multiply_sum_rescale(h, p(out), ops_a, ops_b, None, 2, batch, 1) == HEXL_E_BADARG
        assert lib.hexl_hks_multiply_sum_relinearize(h, p(out), ops_a, ops_b, None, 2, batch, 1) == HEXL_E_NOKEYS    # level 1 is a level
        assert lib.hexl_hks_relinearize_rescale(h, p(out), p(ct3), 1 << 62, L) == HEXL_E_BADARG
    # d_out overlapping an operand or d_ct3 (batch 2)
    for fn in fused:
        assert fn(h, p(a[n:]), ops_a, ops_b, None, 2, 2, L) == HEXL_E_BADARG
        assert fn(h, p(b), ops_a, ops_b, None, 2, 2, L) == HEXL_E_BADARG
    assert lib.hexl_hks_relinearize_rescale(h, p(ct3[n:]), p(ct3), 2, L) == HEXL_E_BADARG
    assert lib.hexl_hks_relinearize_rescale(h, p(ct3), p(ct3), 2, L) == HEXL_E_BADARG
    assert lib.hexl_hks_mul_scratch_bytes(None, 1) == 0
    ctx.sync()
    assert bool((out == -1).all()) and not bool(a.any()) and not bool(b.any()) and not bool(ct3.any()), "a refusal wrote something"
    s.hks.set_keys_device(up(hx, dev, s.keys()))
    for fn in fused:
        assert fn(h, p(out), ops_a, ops_b, None, 2, 0, L) == 0
    assert lib.hexl_hks_relinearize_rescale(h, p(out), p(ct3), 0, L) == 0
    ctx.sync()
    assert bool((out == -1).all()), "an empty batch wrote something"
    # an integer-kernel plan never gets a hybrid object, so no call can reach one
    big = KsCase(orc, n, 2, 4, seed=3, bits=55)
    iplan = hx.KeySwitchPlan(ctx, n, 2, 4, 4, 2, big.moduli, big.modswitch)
    out_h = vp()
    assert lib.hexl_hks_create(iplan.h, 1, ctypes.byref(out_h)) == HEXL_E_BADARG and not out_h.value
    iplan.close()
    s.close()


def test_end_to_end_product_decrypts_and_decodes_within_the_noise_bound(hx, ctx, dev, orc):
    """encode two slot vectors at scale 2^40 and level 3 -> hexl_rlwe_encrypt under a ternary secret -> multiply_sum_rescale with the
    relinearisation key of gen_hybrid_key (s^2 -> s) -> hexl_rlwe_decrypt at level 2 -> decode at scale^2 / q_2.
    With m = the encoded plaintext and e = the CBD21 error of an encryption (|e| <= 21), D(s) = (m_a + e_a)(m_b + e_b), so
        q_2 (out_0 + out_1 s) - m_a m_b = m_a e_b + m_b e_a + e_a e_b + q_2 eps,   |eps| <= B of the definition,
    and the three products are bounded term by term: a negacyclic product of n coefficients, ||x y|| <= n ||x|| ||y||."""
    torch = torch_()
    n, L, K, alpha, l = 1024, 3, 5, 2, 3
    s = Setup(hx, ctx, orc, n, L, K, alpha, orc.primes(K, 45, n))
    hm = mul_model(orc, s)
    plan, qs = s.plan, s.qs
    seed = bytes((29 * k + 5) & 0xFF for k in range(32))
    sec = minus_one(dev, K * n)
    plan.sample(sec, hx.SAMPLE_TERNARY, 1, K, seed=seed, stream=1)
    s2 = minus_one(dev, K * n)
    plan.multiply_plain(s2, sec, sec, 1, 1, K, 1)
    d_keys = minus_one(dev, hm.dnum * 2 * K * n)
    plan.gen_hybrid_key(d_keys, sec, alpha, s2, seed=seed, stream=2)
    s.hks.set_keys_device(d_keys)
    scale = 2.0 ** 40
    rng = np.random.default_rng(5)
    xs = [rng.uniform(-1, 1, (n // 2, 2)) for _ in range(2)]
    pts, cts, mags = [], [], []
    for k, x in enumerate(xs):
        pt, ct, co = minus_one(dev, l * n), minus_one(dev, 2 * l * n), torch.zeros(n, dtype=torch.float64, device=dev)
        plan.ckks_encode(pt, torch.from_numpy(x).to(dev), 1, l, scale)
        plan.rlwe_encrypt(ct, sec, 1, l, pt=pt, seed=seed, stream=3 + k)
        plan.rns_to_f64(co, pt, 1, l)
        pts.append(pt); cts.append(ct); mags.append(co)
    out, dec, mm = minus_one(dev, 2 * (l - 1) * n), minus_one(dev, (l - 1) * n), minus_one(dev, l * n)
    s.hks.multiply_sum_rescale(out, [cts[0]], [cts[1]], 1, l)
    plan.rlwe_decrypt(dec, out, sec, 1, 2, l - 1)
    plan.multiply_plain(mm, pts[0], pts[1], 1, 1, l, 1)           # m_a m_b modulo Q_3, far below Q_3 / 2
    slots = torch.zeros(n // 2, 2, dtype=torch.float64, device=dev)
    q = qs[l - 1]
    plan.ckks_decode(slots, dec, 1, l - 1, scale * scale / q)
    ctx.sync()
    V, _ = hm.crt_coeffs(hx.to_u64(dec).reshape(l - 1, n), list(range(l - 1)), centred=True)
    M, _ = hm.crt_coeffs(hx.to_u64(mm).reshape(l, n), list(range(l)), centred=True)
    ma, mb = (float(c.abs().max().item()) for c in mags)
    B = hm.rescale_noise_bound(l)
    bound = 21 * n * ma + 21 * n * mb + 21 * 21 * n + q * B
    worst = max(abs(q * int(v) - int(m)) for v, m in zip(V, M))
    print(f"[hks multiply] |q dec - m_a m_b| = {worst / q:.2f} q, bound {bound / q:.2f} q (B = {B:.1f}, |m| <= {ma:.3g}, {mb:.3g})")
    assert worst <= bound, f"{worst} > {bound}"
    # the slots: a coefficient error of `bound / q` at scale^2 / q moves a slot by at most n times that; the encodings' own rounding
    # (half a unit per coefficient, n coefficients, at `scale`) moves a product of two slots below 1 by at most 2 n / scale
    got = slots.cpu().numpy()
    za, zb = xs[0][:, 0] + 1j * xs[0][:, 1], xs[1][:, 0] + 1j * xs[1][:, 1]
    err = np.abs((got[:, 0] + 1j * got[:, 1]) - za * zb).max()
    tol = n * (bound / q) / (scale * scale / q) + 2 * n / scale
    print(f"[hks multiply] slot error {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol
    s.close()
