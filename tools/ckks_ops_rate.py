#!/usr/bin/env python3
"""ckks_ops_rate.py [iters = 10] -- device rates of the CKKS level operations (hexl_rescale, hexl_apply_galois, hexl_rotate) after
warm-up, timed with device events on the context's stream, at the headline shape (N = 16384, L = 7, K = 8, GeneratePrimes(8, 51, N):
moduli in (2^51, 2^52), the FP64 kernels) and at bridge-seal's chain (52,30,30,40,27,27,27; L = 6, K = 7):
  rescale/s        L -> L - 1 limbs, 2 components, batch 8192
  apply_galois     GB/s (bytes read + written) next to a torch copy of the same bytes
  rotate/s         next to bare hexl_keyswitch/s on the same plan and batch
Prints one JSON document."""
import json
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]
import torch
import hexl_fpga_amd as hx
import orc
from ks_util import KsCase, seal_chain

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
N = 16384
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


def residues(moduli, reps):
    """[reps][len(moduli)][N] words below their limb's modulus"""
    g = torch.Generator(device=dev).manual_seed(len(moduli) * 7 + reps)
    one = torch.stack([torch.randint(0, int(q), (N,), dtype=torch.int64, device=dev, generator=g) for q in moduli])
    return one.repeat(reps, 1, 1).reshape(-1)


def shape_rows(ctx, name, moduli, L, rs_batch=8192, rot_batch=2048):
    K = len(moduli)
    case = KsCase(orc, N, L, K, seed=3, moduli=moduli)
    plan = hx.KeySwitchPlan(ctx, N, L, K, K, 2, case.moduli, case.modswitch)
    plan.set_keys(case.keys)
    rows = {"shape": name, "n": N, "L": L, "K": K, "moduli_bits": [int(q).bit_length() for q in moduli]}
    # rescale: [batch][2][L][n] -> [batch][2][L - 1][n]
    x = residues(list(moduli[:L]) * 2, rs_batch)
    y = torch.empty(rs_batch * 2 * (L - 1) * N, dtype=torch.int64, device=dev)
    ms = timed(lambda: plan.rescale(y, x, rs_batch, L, 2))
    rows["rescale"] = {"batch": rs_batch, "limbs": [L, L - 1], "components": 2, "ms": ms, "per_s": rs_batch / ms * 1e3,
                       "GBps_min_traffic": rs_batch * 2 * (2 * L - 1) * N * 8 / ms / 1e6}
    del x, y
    # rotate vs keyswitch: same plan, same batch
    ct = residues(list(moduli[:L]) * 2, rot_batch)
    out = torch.empty_like(ct)
    ms_rot = timed(lambda: plan.rotate(out, ct, rot_batch, pow(5, 7, 2 * N)))
    t = ct.view(rot_batch, 2, L * N)[:, 1].contiguous()
    ms_ks = timed(lambda: plan.keyswitch(out, t, rot_batch))       # accumulates into `out`: the rate is what is measured
    rows["rotate"] = {"batch": rot_batch, "ms": ms_rot, "per_s": rot_batch / ms_rot * 1e3}
    rows["keyswitch"] = {"batch": rot_batch, "ms": ms_ks, "per_s": rot_batch / ms_ks * 1e3}
    rows["rotate_over_keyswitch"] = ms_ks / ms_rot
    # apply_galois on the same polynomials vs a torch copy of the same bytes
    polys = rot_batch * 2 * L
    nbytes = 2 * polys * N * 8                                       # read + write
    ms_g = timed(lambda: ctx.apply_galois(out, ct, polys, N, pow(5, 7, 2 * N)))
    ms_c = timed(lambda: out.copy_(ct))
    rows["apply_galois"] = {"polynomials": polys, "ms": ms_g, "GBps": nbytes / ms_g / 1e6}
    rows["torch_copy"] = {"bytes_read_plus_written": nbytes, "ms": ms_c, "GBps": nbytes / ms_c / 1e6}
    plan.close()
    return rows


ctx = hx.Context(0)
result = {"device": ctx.describe(), "iters": ITERS,
          "rows": [shape_rows(ctx, "headline", orc.primes(8, 51, N), 7),
                   shape_rows(ctx, "seal_chain", seal_chain(orc, 7, N), 6)]}
ctx.close()
print(json.dumps(result, indent=1))
