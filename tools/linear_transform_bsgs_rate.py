#!/usr/bin/env python3
"""linear_transform_bsgs_rate.py [iters = 10] [out = profiles/linear_transform_bsgs_rate.json] -- device time of ONE
hexl_linear_transform_bsgs call against the two routes a caller had before it, on the same plans, inputs and plaintexts in the same
process, after warm-up, timed with device events on the context's stream (the shape of tools/linear_transform_rate.py), at N = 16384
on the headline chain (L = 7, K = 8, GeneratePrimes(8, 51, N)) and on bridge-seal's chain (52,30,30,40,27,27,27; L = 6, K = 7), batch
128, for (n_baby, n_giant) = (4, 4) and (8, 8), every diagonal present, no identity terms, G_0 = 1:
  bsgs          one hexl_linear_transform_bsgs call
  composition   the device composition that defines its words: per giant step hexl_linear_transform over the n_baby baby steps, then
                hexl_rotate_hoisted with one rotation (none for G = 1), then a modular add of the result in torch
  flat          one hexl_linear_transform call with n_baby * n_giant rotations, one plan with its own keys per rotation
Baby elements 5^i, giant elements 5^(n_baby j); the flat route's elements are their products. Every figure is the median of `iters`
calls, taken three times (`repeats`), listed lowest to highest. Writes and prints one JSON document."""
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
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "linear_transform_bsgs_rate.json"
N, BATCH, REPEATS, GRIDS = 16384, 128, 3, ((4, 4), (8, 8))
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
    K, dmax = len(moduli), max(b * g for b, g in GRIDS)
    plans = []
    for r in range(dmax):                                              # the flat route needs one plan per diagonal
        case = KsCase(orc, N, L, K, seed=3 + r, moduli=moduli)
        plans.append(hx.KeySwitchPlan(ctx, N, L, K, K, 2, case.moduli, case.modswitch))
        plans[-1].set_keys(case.keys)
    g = torch.Generator(device=dev).manual_seed(L)
    words = lambda qs: torch.stack([torch.randint(0, int(q), (N,), dtype=torch.int64, device=dev, generator=g) for q in qs])
    ct = words(list(moduli[:L]) * 2).repeat(BATCH, 1, 1).reshape(-1)
    pts = [words(list(moduli[:L]) + [moduli[K - 1]]).reshape(-1) for _ in range(dmax)]
    q = torch.tensor([int(v) for v in moduli[:L]], dtype=torch.int64, device=dev).reshape(1, 1, L, 1)
    out_b, out_c, out_f, t, r_ = (torch.empty_like(ct) for _ in range(5))
    rows = {"shape": name, "n": N, "L": L, "K": K, "batch": BATCH, "moduli_bits": [int(v).bit_length() for v in moduli],
            "tiers": plans[0].tiers()[0], "by_grid": []}
    for nb_, ng in GRIDS:
        bgs = [pow(5, i, 2 * N) for i in range(nb_)]
        ggs = [pow(5, nb_ * j, 2 * N) for j in range(ng)]
        bplans, gplans = plans[:nb_], [None] + plans[nb_:nb_ + ng - 1]
        grid = [[pts[j * nb_ + i] for i in range(nb_)] for j in range(ng)]
        flat_gs = [bgs[i] * ggs[j] % (2 * N) for j in range(ng) for i in range(nb_)]

        def composition():
            for j in range(ng):
                dst = out_c if j == 0 else t
                hx.linear_transform(bplans, bgs, grid[j], dst, ct, BATCH)
                if ggs[j] != 1:
                    hx.rotate_hoisted([gplans[j]], [ggs[j]], [r_], dst, BATCH)
                    s = out_c.view(BATCH, 2, L, N) + r_.view(BATCH, 2, L, N)
                    out_c.view(BATCH, 2, L, N).copy_(torch.where(s >= q, s - q, s))

        a = sorted(timed(lambda: hx.linear_transform_bsgs(bplans, bgs, gplans, ggs, grid, out_b, ct, BATCH)) for _ in range(REPEATS))
        b = sorted(timed(composition) for _ in range(REPEATS))
        c = sorted(timed(lambda: hx.linear_transform(plans[:nb_ * ng], flat_gs, pts[:nb_ * ng], out_f, ct, BATCH)) for _ in range(REPEATS))
        assert torch.equal(out_b, out_c), "the call and the device composition must agree word for word"
        rows["by_grid"].append({"n_baby": nb_, "n_giant": ng, "bsgs_ms": a, "composition_ms": b, "flat_ms": c,
                                "bsgs_scratch_bytes": hx.lt_bsgs_scratch_bytes(plans[0], nb_, BATCH),
                                "ratio_composition_over_bsgs": [y / x for x, y in zip(a, b)],
                                "ratio_flat_over_bsgs": [y / x for x, y in zip(a, c)]})
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
