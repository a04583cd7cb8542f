#!/usr/bin/env python3
"""hks_bsgs_rate.py [iters = 5] [out = profiles/hks_bsgs_rate.json] -- one hexl_hks_linear_transform_bsgs call against the routes it
replaces, at N = 16384 on 51-bit primes, for (n_baby, n_giant) = (4, 4) and (8, 8) with the first giant step G = 1, at two shapes:
    L = 12, alpha = 4, n_p = 4          L = 7, alpha = 2, n_p = 2
    bsgs         one hexl_hks_linear_transform_bsgs call, n_baby + n_giant - 1 keyed objects
    composition  the device composition that defines its words: hexl_hks_linear_transform per row, hexl_hks_rotate_hoisted per rotated
                 giant step, a modular add (torch) per row
    flat         one hexl_hks_linear_transform over n_baby x n_giant keyed objects (the composed elements g_i G_j)
    bsgs_sparse  the same call with ONE plaintext per row (every baby column still used): the difference to `bsgs`, divided by the
                 n_giant (n_baby - 1) terms left out, is the cost of one more term of a row -- k_hks_bsgs_sum's two stored vectors and
                 k_galois_c0_pt's gather of c0 together -- beside the flat route's own cost of one more term at this batch,
                 (flat 8 x 8 - flat 4 x 4) / 48, which is k_hks_mac<., PT_ACC> and the same gather (DESIGN.md 4.6.11 measured
                 0.40 ms per term at batch 128)
The batch is 64: the baby store of 8 steps at K = 16 is 32 MiB per instance, so 64 instances fill its 2 GiB and run as one chunk.
Every (shape, grid) runs in a child process of its own under a time limit, all its routes in that one process; this process never opens
the device and stops at the first child that fails. Every figure is the median of `iters` calls, taken three times with the routes
alternating; a ratio > 1 means the bsgs call is FASTER by that factor. The child asserts that the call equals the composition word for
word at that size. Keys, ciphertexts and plaintexts are uniform words (hexl_sample). No ratio is promised."""
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
    sparse = [[pts[j][i] if i == j % n_baby else None for i in range(n_baby)] for j in range(n_giant)]
    flat_pts = [p for row in pts for p in row]
    ct = uniform(2 * BATCH, L, 1)
    out, total, t, r, flat_out = (torch.empty_like(ct) for _ in range(5))
    q = torch.tensor([int(v) for v in moduli[:L]], dtype=torch.int64, device=dev).reshape(1, 1, L, 1)
    shape = (BATCH, 2, L, N)

    def composition():
        for j, G in enumerate(ggs):
            hx.hks_linear_transform(baby, bgs, pts[j], None, t, ct, BATCH, L)
            src = t
            if G != 1:
                hx.hks_rotate_hoisted([giant[j]], [G], [r], t, BATCH, L)
                src = r
            if j == 0:
                total.copy_(src)
            else:
                v = total.view(shape)
                v.add_(src.view(shape))
                v.sub_(torch.where(v >= q, q, torch.zeros_like(q)))

    routes = {"bsgs": lambda: hx.hks_linear_transform_bsgs(baby, bgs, giant, ggs, pts, None, out, ct, BATCH, L),
              "composition": composition,
              "flat": lambda: hx.hks_linear_transform(flat_objs, flat_gs, flat_pts, None, flat_out, ct, BATCH, L),
              "bsgs_sparse": lambda: hx.hks_linear_transform_bsgs(baby, bgs, giant, ggs, sparse, None, out, ct, BATCH, L)}
    routes["composition"]()
    routes["bsgs"]()
    ctx.sync()
    assert torch.equal(out, total), "the call is not the device composition word for word"
    ms = {k: [] for k in routes}
    for _ in range(REPEATS):
        for k, fn in routes.items():
            ms[k].append(timed(fn))
    key_bytes = dnum * 2 * K * N * 8
    digits = [min(alpha, L - d * alpha) for d in range(dnum)]
    U, D = L + sum(L + n_p - g for g in digits), 2 * n_p + 2 * L
    rot = sum(1 for G in ggs if G != 1)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    row = {"L": L, "alpha": alpha, "n_p": n_p, "K": K, "dnum": dnum, "batch": BATCH, "n_baby": n_baby, "n_giant": n_giant, "ms": ms,
           "bsgs_over_composition": [a / b for a, b in zip(ms["composition"], ms["bsgs"])],
           "bsgs_over_flat": [a / b for a, b in zip(ms["flat"], ms["bsgs"])],
           "keys_held_bytes": {"bsgs": (n_baby + rot) * key_bytes, "flat": n_baby * n_giant * key_bytes},
           "transforms_per_instance": {"flat": U + D, "composition": (n_giant + rot) * (U + D), "bsgs": U + n_giant * D + rot * (U + D)},
           "key_passes": {"flat": n_baby * n_giant, "bsgs": n_baby + rot},
           "ms_per_row_term_sum_and_c0_kernels": (med(ms["bsgs"]) - med(ms["bsgs_sparse"])) / (n_giant * (n_baby - 1)),
           "pt_acc_ms_per_term_design_4_6_11": 0.40,
           "word_identical_to_composition": True,
           "bsgs_scratch_bytes": baby[0].bsgs_scratch_bytes(n_baby, BATCH), "device": ctx.describe()}
    print("ROW " + json.dumps(row), flush=True)
    for o in reversed(baby + [g for g in giant if g is not None] + flat_objs):
        o.close()
    plan.close()
    ctx.close()


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "hks_bsgs_rate.json"
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
    # one more term of the FLAT route at this batch, from its own two grids: (flat at 8 x 8 - flat at 4 x 4) / (64 - 16) terms
    med = lambda xs: sorted(xs)[len(xs) // 2]
    flat_term = {}
    for L, alpha, n_p in SHAPES:
        of = {(r["n_baby"], r["n_giant"]): med(r["ms"]["flat"]) for r in rows if (r["L"], r["alpha"]) == (L, alpha)}
        flat_term[f"L{L}_alpha{alpha}"] = (of[GRIDS[1]] - of[GRIDS[0]]) / (GRIDS[1][0] * GRIDS[1][1] - GRIDS[0][0] * GRIDS[0][1])
    device = rows[0]["device"]
    for row in rows:
        del row["device"]
    result = {"what": "one run on one machine", "device": device, "iters": iters, "repeats": REPEATS, "n": N, "moduli_bits": 51,
              "flat_ms_per_further_term_at_this_batch": flat_term, "rows": rows}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*map(int, sys.argv[2:8]))
    else:
        main()
