#!/usr/bin/env python3
"""hks_rate.py [iters = 5] [out = profiles/hks_rate.json] -- the hybrid key switch (hexl_hks_keyswitch) against the per-limb gadget
(hexl_keyswitch) in ONE process at N = 16384, on plans with the same data limbs (GeneratePrimes(., 51, N)), batch = one scratch chunk
(256 instances), timed with device events on the context's stream after warm-up:
    L = 7   alpha = 1, 2, 4      L = 12   alpha = 3, 4, 6      n_p = min(alpha, 16 - L) special primes (P ~ the largest digit,
                                                               except alpha = 6 at L = 12: K is at most 16, so n_p = 4)
The per-limb route has K = L + 1 and runs the library's production pipeline for that batch; the hybrid route runs its own
one-transform-per-workgroup kernels. Keys and operands are uniform words (hexl_sample): a key switch's time does not depend on them.
Every figure is the median of `iters` calls, taken three times (`repeats`) with the routes alternating, so the spread is on record;
`hybrid_over_per_limb` > 1 means the hybrid route is SLOWER. Transform and key-word counts are the formulas of DESIGN.md 4.6.10.
Writes and prints one JSON document. No ratio is promised: the crossover L is the finding."""
import json
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]
import torch
import hexl_fpga_amd as hx
import orc

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "hks_rate.json"
N, BATCH, REPEATS = 16384, 256, 3
SHAPES = [(7, 1), (7, 2), (7, 4), (12, 3), (12, 4), (12, 6)]
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
primes = orc.primes(12 + 6, 51, N)
rows = []
per_limb_ms = {}
for L, alpha in SHAPES:
    n_p, dnum = min(alpha, 16 - L), -(-L // alpha)                # (a plan has at most 16 limbs: alpha = 6 at L = 12 gets n_p = 4)
    K = L + n_p
    data, special = primes[:L], primes[12:12 + n_p]
    # the per-limb plan of these data limbs: K = L + 1
    pm = list(data) + [special[0]]
    msw = [pow(int(pm[-1]), -1, int(q)) for q in pm[:-1]] + [1]
    plan1 = hx.KeySwitchPlan(ctx, N, L, L + 1, L + 1, 2, pm, msw)
    plan1.set_keys_device(uniform(plan1, 2 * L, L + 1, 1))
    hm = list(data) + list(special)
    planh = hx.KeySwitchPlan(ctx, N, L, K, K, 2, hm, [pow(int(hm[-1]), -1, int(q)) for q in hm[:-1]] + [1])
    hks = hx.HybridKeySwitch(planh, alpha)
    hks.set_keys_device(uniform(planh, 2 * dnum, K, 2))
    t = uniform(plan1, BATCH, L, 3)
    r1, rh = uniform(plan1, 2 * BATCH, L, 4), uniform(plan1, 2 * BATCH, L, 4)
    routes = {"per_limb": lambda: plan1.keyswitch(r1, t, BATCH), "hybrid": lambda: hks.keyswitch(rh, t, BATCH, L)}
    ms = {k: [] for k in routes}
    for _ in range(REPEATS):
        for k, fn in routes.items():
            ms[k].append(timed(fn))
    digits = [min(alpha, L - d * alpha) for d in range(dnum)]
    rows.append({"L": L, "alpha": alpha, "n_p": n_p, "dnum": dnum, "K": K, "batch": BATCH,
                 "hybrid_transforms": L + sum(L + n_p - g for g in digits) + 2 * n_p + 2 * L, "per_limb_transforms": L * L + 3 * L + 2,
                 "hybrid_key_words_over_n": dnum * 2 * K, "per_limb_key_words_over_n": L * 2 * (L + 1),
                 "ms": ms, "keyswitch_per_s": {k: [BATCH / m * 1e3 for m in v] for k, v in ms.items()},
                 "hybrid_over_per_limb": [h / p for h, p in zip(ms["hybrid"], ms["per_limb"])],
                 "scratch_bytes": {"hybrid": hks.scratch_bytes(BATCH), "per_limb": plan1.scratch_bytes(BATCH)}})
    print(json.dumps(rows[-1]), flush=True)
    hks.close()
    planh.close()
    plan1.close()
    del t, r1, rh
    torch.cuda.empty_cache()
result = {"device": ctx.describe(), "iters": ITERS, "repeats": REPEATS, "n": N, "moduli_bits": 51, "rows": rows}
ctx.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
