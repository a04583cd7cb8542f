#!/usr/bin/env python3
"""linear_transform_rate.py [iters = 10] [out = profiles/linear_transform_rate.json] -- device time of ONE hexl_linear_transform call
against the three-call route it replaces -- hexl_rotate_hoisted followed by R x hexl_multiply_plain(accumulate) -- on the same plans,
inputs and outputs in the same process, after warm-up, timed with device events on the context's stream (the shape of
tools/rotate_hoisted_rate.py), at N = 16384 on the headline chain (L = 7, K = 8, GeneratePrimes(8, 51, N)) and on bridge-seal's chain
(52,30,30,40,27,27,27; L = 6, K = 7), for R = 1, 2, 4, 8, 16 rotations (g = 5^k, k = 1 ... R, one plan with its own keys per rotation)
of a batch of 128 ciphertexts: one scratch chunk.
  transforms/s  R x batch plaintext-weighted rotations per call, and the ratio three-call time / linear-transform time
The three-call route's first product is written (accumulate = 0), the others are added. Every figure is the median of `iters` calls,
taken three times (`repeats`), listed lowest to highest. Writes and prints one JSON document."""
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
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "linear_transform_rate.json"
N, BATCH, REPEATS, ROTATIONS = 16384, 128, 3, (1, 2, 4, 8, 16)
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


def shape_rows(ctx, name, moduli, L):
    K, rmax = len(moduli), max(ROTATIONS)
    cases = [KsCase(orc, N, L, K, seed=3 + r, moduli=moduli) for r in range(rmax)]
    plans = []
    for case in cases:
        plans.append(hx.KeySwitchPlan(ctx, N, L, K, K, 2, case.moduli, case.modswitch))
        plans[-1].set_keys(case.keys)
    gs = [pow(5, k + 1, 2 * N) for k in range(rmax)]
    g = torch.Generator(device=dev).manual_seed(L)
    words = lambda qs: torch.stack([torch.randint(0, int(q), (N,), dtype=torch.int64, device=dev, generator=g) for q in qs])
    ct = words(list(moduli[:L]) * 2).repeat(BATCH, 1, 1).reshape(-1)
    pts = [words(list(moduli[:L]) + [moduli[K - 1]]).reshape(-1) for _ in range(rmax)]     # [L + 1][n]; the three-call route reads rows 0 ... L - 1
    rot = [torch.empty_like(ct) for _ in range(rmax)]
    out_lt, out_3 = torch.empty_like(ct), torch.empty_like(ct)
    rows = {"shape": name, "n": N, "L": L, "K": K, "batch": BATCH, "moduli_bits": [int(q).bit_length() for q in moduli],
            "tiers": plans[0].tiers()[0], "by_rotations": []}

    def three_calls(R):
        hx.rotate_hoisted(plans[:R], gs[:R], rot[:R], ct, BATCH)
        for r in range(R):
            plans[0].multiply_plain(out_3, rot[r], pts[r], BATCH, 2, L, 1, accumulate=r > 0)

    for R in ROTATIONS:
        a = sorted(timed(lambda: hx.linear_transform(plans[:R], gs[:R], pts[:R], out_lt, ct, BATCH)) for _ in range(REPEATS))
        b = sorted(timed(lambda: three_calls(R)) for _ in range(REPEATS))
        per_s = lambda ms: [R * BATCH / m * 1e3 for m in ms]
        rows["by_rotations"].append({"R": R, "linear_transform_ms": a, "three_calls_ms": b, "linear_transform_per_s": per_s(a),
                                     "three_calls_per_s": per_s(b), "ratio_three_calls_over_linear_transform": [y / x for x, y in zip(a, b)]})
    assert all(p.range_check() for p in plans)
    for p in plans:
        p.close()
    return rows


ctx = hx.Context(0)
result = {"device": ctx.describe(), "iters": ITERS, "repeats": REPEATS,
          "rows": [shape_rows(ctx, "headline", orc.primes(8, 51, N), 7),
                   shape_rows(ctx, "seal_chain", seal_chain(orc, 7, N), 6)]}
ctx.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
