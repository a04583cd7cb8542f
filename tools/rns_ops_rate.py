#!/usr/bin/env python3
"""rns_ops_rate.py [iters = 10] [out = profiles/rns_ops_rate.json] -- device rates of hexl_rns_ntt_fwd / hexl_rns_ntt_inv and
hexl_multiply_plain after warm-up, timed with device events on the context's stream (the shape of tools/ckks_ops_rate.py), at N = 16384 on
the headline chain (L = 7, K = 8, GeneratePrimes(8, 51, N)) and on bridge-seal's chain (52,30,30,40,27,27,27; L = 6, K = 7):
  polynomials/s    hexl_rns_ntt_fwd / _inv, count = 2048 x 2, n_limbs = L, next to hexl_ntt_fwd / hexl_ntt_inv in the same process on the
                   same number of polynomials and one prime of the chain's most common tier
  TB/s             hexl_multiply_plain, batch 2048, 2 components, pt_batch 1 and batch, with and without accumulate, in bytes that must
                   move (ct read, out written, pt read once per instance it belongs to, out read when accumulating), next to
                   hexl_dyadic_multiply on the same ciphertexts and a torch copy of the ciphertext
Every figure is the median of `iters` calls, taken three times (`repeats`), so the spread is on record. Writes and prints one JSON document."""
import json
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]
import numpy as np
import torch
import hexl_fpga_amd as hx
import orc
from ks_util import KsCase, seal_chain

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "rns_ops_rate.json"
N, BATCH, REPEATS = 16384, 2048, 3
dev = torch.device("cuda:0")


def timed(fn, iters=ITERS, warmup=2):
    """median milliseconds per call over `iters` calls, each bracketed by events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return 0.5 * (ms[(len(ms) - 1) // 2] + ms[len(ms) // 2])


def repeated(fn, unit):
    """{'ms': [three medians], key: [the rate of each]}; unit = (key, amount per call) -> amount / second"""
    ms = [timed(fn) for _ in range(REPEATS)]
    key, amount = unit
    return {"ms": ms, key: [amount / m * 1e3 for m in ms]}


def residues(moduli, reps):
    """[reps][len(moduli)][N] words below their limb's modulus"""
    g = torch.Generator(device=dev).manual_seed(len(moduli) * 7 + reps)
    one = torch.stack([torch.randint(0, int(q), (N,), dtype=torch.int64, device=dev, generator=g) for q in moduli])
    return one.repeat(reps, 1, 1).reshape(-1)


def shape_rows(ctx, name, moduli, L):
    K = len(moduli)
    case = KsCase(orc, N, L, K, seed=3, moduli=moduli)
    plan = hx.KeySwitchPlan(ctx, N, L, K, K, 2, case.moduli, case.modswitch)
    tiers = plan.tiers()[0]
    rows = {"shape": name, "n": N, "L": L, "K": K, "moduli_bits": [int(q).bit_length() for q in moduli], "tiers": tiers}
    # transforms: [count][L][n], count = batch x 2 components
    count, polys = BATCH * 2, BATCH * 2 * L
    x = residues(list(moduli[:L]), count)
    y = torch.empty_like(x)
    rows["rns_ntt_fwd"] = dict(polynomials=polys, **repeated(lambda: plan.rns_ntt_fwd(y, x, count, L), ("per_s", polys)))
    rows["rns_ntt_inv"] = dict(polynomials=polys, **repeated(lambda: plan.rns_ntt_inv(y, x, count, L), ("per_s", polys)))
    rows["rns_ntt_fwd_in_place"] = dict(polynomials=polys, **repeated(lambda: plan.rns_ntt_fwd(x, x, count, L), ("per_s", polys)))
    # the standalone kernels on as many polynomials of one modulus: the limb whose tier most limbs in use share
    common = max(set(tiers[:L]), key=tiers[:L].count)
    i = tiers[:L].index(common)
    q = int(moduli[i])
    t = orc.HexlTables(N, q)
    tabs = [hx.as_i64(a).to(dev) for a in (t.roots, t.precon, t.inv_roots, t.inv_precon)]
    x = residues([q], polys)
    rows["ntt_fwd"] = dict(polynomials=polys, modulus_bits=q.bit_length(), tier=common,
                           **repeated(lambda: ctx.ntt_fwd(x, tabs[0], tabs[1], q, N), ("per_s", polys)))
    rows["ntt_inv"] = dict(polynomials=polys, modulus_bits=q.bit_length(), tier=common,
                           **repeated(lambda: ctx.ntt_inv(x, tabs[2], tabs[3], q, t.inv_n, t.inv_n_w, N), ("per_s", polys)))
    del x, y
    # plaintext multiply: [batch][2][L][n] by [pt_batch][L][n]
    ct = residues(list(moduli[:L]) * 2, BATCH)
    pts = residues(list(moduli[:L]), BATCH)
    out = residues(list(moduli[:L]) * 2, BATCH)
    ct_bytes, pt_bytes = BATCH * 2 * L * N * 8, L * N * 8
    for per_instance in (False, True):
        for acc in (False, True):
            nbytes = ct_bytes * (3 if acc else 2) + pt_bytes * (BATCH if per_instance else 1)
            key = f"multiply_plain_pt_{'batch' if per_instance else '1'}{'_accumulate' if acc else ''}"
            rows[key] = dict(bytes_min=nbytes, **repeated(
                lambda: plan.multiply_plain(out, ct, pts, BATCH, 2, L, BATCH if per_instance else 1, accumulate=acc), ("TBps", nbytes / 1e12)))
    rows["torch_copy"] = dict(bytes_read_plus_written=2 * ct_bytes, **repeated(lambda: out.copy_(ct), ("TBps", 2 * ct_bytes / 1e12)))
    out3 = torch.empty(BATCH * 3 * L * N, dtype=torch.int64, device=dev)
    d_mod = hx.as_i64(np.tile(case.moduli[:L], BATCH)).to(dev)       # [batch][n_moduli]
    dy_bytes = BATCH * 7 * L * N * 8                               # two operands of two components read, three components written
    rows["dyadic_multiply"] = dict(bytes_min=dy_bytes, **repeated(lambda: ctx.dyadic_multiply(out3, ct, out, d_mod, N, L), ("TBps", dy_bytes / 1e12)))
    plan.close()
    return rows


ctx = hx.Context(0)
result = {"device": ctx.describe(), "iters": ITERS, "repeats": REPEATS, "batch": BATCH,
          "rows": [shape_rows(ctx, "headline", orc.primes(8, 51, N), 7),
                   shape_rows(ctx, "seal_chain", seal_chain(orc, 7, N), 6)]}
ctx.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
