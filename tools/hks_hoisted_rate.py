#!/usr/bin/env python3
"""hks_hoisted_rate.py [iters = 5] [out = profiles/hks_hoisted_rate.json] -- the hoisted calls on the hybrid key switch against the routes
they replace, in ONE process at N = 16384 on 51-bit primes (GeneratePrimes(., 51, N)), batch 128 (one scratch chunk), timed with device
events on the context's stream after warm-up, for R = 1, 2, 4, 8, 16 rotations of one ciphertext batch with R keyed objects on one plan:
    L = 12, alpha = 4, n_p = 4          L = 7, alpha = 2, n_p = 2
    hoisted    one hexl_hks_rotate_hoisted call              against  R calls of hexl_hks_rotate
    transform  one hexl_hks_linear_transform call            against  hexl_hks_rotate_hoisted + R x hexl_multiply_plain(accumulate)
Keys, ciphertexts and plaintexts are uniform words (hexl_sample): the time of these calls does not depend on them. Every figure is the
median of `iters` calls, taken three times (`repeats`) with the routes alternating, so the spread is on record; a ratio > 1 means the
single call is FASTER by that factor. `expected_by_transforms` is the ratio of transform counts per instance: with
up = l + sum_d (l + n_p - |G_d|) and down = 2 n_p + 2 l, R (up + down) / (up + R down) for the hoisted call and (up + R down) / (up + down)
for the transform against the composed route. Writes and prints one JSON document. No ratio is promised."""
import json
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]
import torch
import hexl_fpga_amd as hx
import orc

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "hks_hoisted_rate.json"
N, BATCH, REPEATS = 16384, 128, 3
SHAPES = [(12, 4, 4), (7, 2, 2)]
ROTATIONS = [1, 2, 4, 8, 16]
SEED = bytes(range(32))
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


def uniform(plan, count, limbs, stream):
    t = torch.empty(count * limbs * N, dtype=torch.int64, device=dev)
    plan.sample(t, hx.SAMPLE_UNIFORM, count, limbs, seed=SEED, stream=stream)
    return t


ctx = hx.Context(0)
rows = []
for L, alpha, n_p in SHAPES:
    K, dnum, R_MAX = L + n_p, -(-L // alpha), max(ROTATIONS)
    moduli = orc.primes(K, 51, N)
    plan = hx.KeySwitchPlan(ctx, N, L, K, K, 2, moduli, [pow(int(moduli[-1]), -1, int(q)) for q in moduli[:-1]] + [1])
    objs = [hx.HybridKeySwitch(plan, alpha) for _ in range(R_MAX)]
    for r, o in enumerate(objs):
        o.set_keys_device(uniform(plan, 2 * dnum, K, 10 + r))
    elts = [pow(5, r + 1, 2 * N) for r in range(R_MAX)]
    ct = uniform(plan, 2 * BATCH, L, 1)
    pts = [uniform(plan, 1, K, 40 + r) for r in range(R_MAX)]
    outs = [torch.empty_like(ct) for _ in range(R_MAX)]
    total = torch.empty_like(ct)
    digits = [min(alpha, L - d * alpha) for d in range(dnum)]
    t_up, t_down = L + sum(L + n_p - g for g in digits), 2 * n_p + 2 * L
    for R in ROTATIONS:
        hs, gs, os_, ps = objs[:R], elts[:R], outs[:R], pts[:R]

        def r_calls():
            for h, g, o in zip(hs, gs, os_):
                h.rotate(o, ct, BATCH, L, g)

        def composed():
            hx.hks_rotate_hoisted(hs, gs, os_, ct, BATCH, L)
            for r in range(R):
                plan.multiply_plain(total, os_[r], ps[r], BATCH, 2, L, 1, accumulate=r > 0)

        routes = {"r_calls_of_rotate": r_calls, "rotate_hoisted": lambda: hx.hks_rotate_hoisted(hs, gs, os_, ct, BATCH, L),
                  "hoisted_plus_multiply_plain": composed,
                  "linear_transform": lambda: hx.hks_linear_transform(hs, gs, ps, None, total, ct, BATCH, L)}
        ms = {k: [] for k in routes}
        for _ in range(REPEATS):
            for k, fn in routes.items():
                ms[k].append(timed(fn))
        rows.append({"L": L, "alpha": alpha, "n_p": n_p, "dnum": dnum, "K": K, "batch": BATCH, "rotations": R,
                     "transforms": {"r_calls_of_rotate": R * (t_up + t_down), "rotate_hoisted": t_up + R * t_down, "linear_transform": t_up + t_down},
                     "ms": ms,
                     "hoisted_speedup": [a / b for a, b in zip(ms["r_calls_of_rotate"], ms["rotate_hoisted"])],
                     "transform_speedup": [a / b for a, b in zip(ms["hoisted_plus_multiply_plain"], ms["linear_transform"])],
                     "expected_by_transforms": {"hoisted": R * (t_up + t_down) / (t_up + R * t_down), "transform": (t_up + R * t_down) / (t_up + t_down)},
                     "hoisted_scratch_bytes": objs[0].hoisted_scratch_bytes(BATCH)})
        print(json.dumps(rows[-1]), flush=True)
    for o in reversed(objs):
        o.close()
    plan.close()
    del ct, pts, outs, total
    torch.cuda.empty_cache()
result = {"device": ctx.describe(), "iters": ITERS, "repeats": REPEATS, "n": N, "moduli_bits": 51, "rows": rows}
ctx.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
