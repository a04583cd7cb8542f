#!/usr/bin/env python3
"""hks_bsgs_ext_rate.py [iters = 5] [out = profiles/hks_bsgs_ext_rate.json] -- one hexl_hks_linear_transform_bsgs_ext call against
hexl_hks_linear_transform_bsgs and the flat hexl_hks_linear_transform, on the shapes, grids, batch and median scheme of
tools/hks_bsgs_rate.py: N = 16384 on 51-bit primes, (n_baby, n_giant) = (4, 4) and (8, 8) with the first giant step G = 1, at
    L = 12, alpha = 4, n_p = 4          L = 7, alpha = 2, n_p = 2
    ext0, ext1          this call with rescale = 0 and rescale = 1 (the rescale folded into the one mod-down)
    ext0_rescale        rescale = 0 followed by hexl_rescale: what ext1 replaces
    bsgs, bsgs_rescale  hexl_hks_linear_transform_bsgs alone and followed by hexl_rescale
    flat, flat_rescale  one hexl_hks_linear_transform over n_baby x n_giant keyed objects, alone and followed by hexl_rescale
Every (shape, grid) runs in a child process of its own under a time limit, all its routes in that one process; this process never opens
the device and stops at the first child that fails. Every figure is the median of `iters` calls, taken three times with the routes
alternating; a ratio > 1 means the ext call is FASTER by that factor. Beside the times stands the prediction by transform count
(U + #{G != 1} (D/2 + U) + D against U + n_giant D + #{G != 1} (U + D), and U + D for flat). Keys, ciphertexts and plaintexts are uniform
words (hexl_sample). No ratio is promised."""
import json
import subprocess
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]

N, BATCH, REPEATS = 16384, 64, 3
SHAPES = [(12, 4, 4), (7, 2, 2)]
GRIDS = [(4, 4), (8, 8)]
CHILD_LIMIT_S = 240


def child(L, alpha, n_p, n_baby, n_giant, iters):
    import torch
    import hexl_fpga_amd as hx
    import orc
    dev = torch.device("cuda:0")
    seed = bytes(range(32))

    def timed(fn, warmup=1):
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

    ctx = hx.Context(0)
    K, dnum = L + n_p, -(-L // alpha)
    moduli = orc.primes(K, 51, N)
    plan = hx.KeySwitchPlan(ctx, N, L, K, K, 2, moduli, [pow(int(moduli[-1]), -1, int(q)) for q in moduli[:-1]] + [1])

    def uniform(count, limbs, stream):
        t = torch.empty(count * limbs * N, dtype=torch.int64, device=dev)
        plan.sample(t, hx.SAMPLE_UNIFORM, count, limbs, seed=seed, stream=stream)
        return t

    def keyed(stream):
        o = hx.HybridKeySwitch(plan, alpha)
        o.set_keys_device(uniform(2 * dnum, K, stream))
        return o

    bgs = [pow(5, i + 1, 2 * N) for i in range(n_baby)]
    ggs = [pow(5, (n_baby + 1) * j, 2 * N) for j in range(n_giant)]          # G_0 = 1
    baby = [keyed(10 + i) for i in range(n_baby)]
    giant = [None] + [keyed(100 + j) for j in range(1, n_giant)]
    flat_objs = [keyed(200 + r) for r in range(n_baby * n_giant)]
    flat_gs = [g * G % (2 * N) for G in ggs for g in bgs]
    pts = [[uniform(1, K, 1000 + j * n_baby + i) for i in range(n_baby)] for j in range(n_giant)]
    flat_pts = [p for row in pts for p in row]
    ct = uniform(2 * BATCH, L, 1)
    out = torch.empty_like(ct)
    low = torch.empty(BATCH * 2 * (L - 1) * N, dtype=torch.int64, device=dev)

    ext = lambda rescale: hx.hks_linear_transform_bsgs_ext(baby, bgs, giant, ggs, pts, None, low if rescale else out, ct, BATCH, L, rescale)
    bsgs = lambda: hx.hks_linear_transform_bsgs(baby, bgs, giant, ggs, pts, None, out, ct, BATCH, L)
    flat = lambda: hx.hks_linear_transform(flat_objs, flat_gs, flat_pts, None, out, ct, BATCH, L)
    then_rescale = lambda fn: lambda: (fn(), plan.rescale(low, out, BATCH, L, 2))
    routes = {"ext0": lambda: ext(0), "ext1": lambda: ext(1), "ext0_rescale": then_rescale(lambda: ext(0)),
              "bsgs": bsgs, "bsgs_rescale": then_rescale(bsgs), "flat": flat, "flat_rescale": then_rescale(flat)}
    ms = {k: [] for k in routes}
    for _ in range(REPEATS):
        for k, fn in routes.items():
            ms[k].append(timed(fn))
    digits = [min(alpha, L - d * alpha) for d in range(dnum)]
    U, D = L + sum(L + n_p - g for g in digits), 2 * n_p + 2 * L
    rot = sum(1 for G in ggs if G != 1)
    counts = {"flat": U + D, "bsgs": U + n_giant * D + rot * (U + D), "ext": U + rot * (D // 2 + U) + D}
    ratio = lambda a, b: [x / y for x, y in zip(ms[a], ms[b])]
    row = {"L": L, "alpha": alpha, "n_p": n_p, "K": K, "dnum": dnum, "batch": BATCH, "n_baby": n_baby, "n_giant": n_giant, "ms": ms,
           "ext0_over_bsgs": ratio("bsgs", "ext0"), "ext0_over_flat": ratio("flat", "ext0"),
           "ext1_over_bsgs_rescale": ratio("bsgs_rescale", "ext1"), "ext1_over_flat_rescale": ratio("flat_rescale", "ext1"),
           "ext1_over_ext0_rescale": ratio("ext0_rescale", "ext1"),
           "transforms_per_instance": counts, "predicted_ext_over_bsgs_by_count": counts["bsgs"] / counts["ext"],
           "bsgs_ext_scratch_bytes": [baby[0].bsgs_ext_scratch_bytes(n_baby, BATCH, r) for r in (0, 1)],
           "bsgs_scratch_bytes": baby[0].bsgs_scratch_bytes(n_baby, BATCH), "device": ctx.describe()}
    print("ROW " + json.dumps(row), flush=True)
    for o in reversed(baby + [g for g in giant if g is not None] + flat_objs):
        o.close()
    plan.close()
    ctx.close()


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "hks_bsgs_ext_rate.json"
    rows = []
    for L, alpha, n_p in SHAPES:
        for n_baby, n_giant in GRIDS:
            cmd = [sys.executable, __file__, "--child", *map(str, (L, alpha, n_p, n_baby, n_giant, iters))]
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
            line = next((x for x in run.stdout.splitlines() if x.startswith("ROW ")), None)
            if run.returncode != 0 or line is None:
                print(run.stdout[-2000:], run.stderr[-3000:])
                raise SystemExit(f"L = {L}, {n_baby} x {n_giant}: the child ended with status {run.returncode}; nothing more is started")
            rows.append(json.loads(line[4:]))
            print(line[4:], flush=True)
    device = rows[0]["device"]
    for row in rows:
        del row["device"]
    result = {"what": "one run on one machine", "device": device, "iters": iters, "repeats": REPEATS, "n": N, "moduli_bits": 51, "rows": rows}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*map(int, sys.argv[2:8]))
    else:
        main()
