#!/usr/bin/env python3
"""hks_multiply_rate.py [iters = 5] [out = profiles/hks_multiply_rate.json] -- products per second of the hybrid multiply
(hexl_hks_multiply_sum_rescale) against the three-call route it replaces, in ONE process on the same buffers, at N = 16384, L = 12,
alpha = 4, n_p = 4 (K = 16, GeneratePrimes(16, 51, N)), batch = one scratch chunk (256 instances), at the full level l = 12 and at l = 6,
for sums of 1 and 4 products, timed with device events on the context's stream after warm-up (the shape of tools/tensor_relin_rate.py):
  fused        one hexl_hks_multiply_sum_rescale: the tensor kernel into the object's buffers, steps 1-3, ONE mod-down by P q_(l-1)
  three_call   hexl_ct_tensor_sum -> hexl_hks_relinearize -> hexl_rescale (NOT word-identical to `fused`: two roundings against one;
               both decrypt alike)
  two_call     hexl_ct_tensor_sum -> hexl_hks_relinearize_rescale (word for word `fused`, asserted here before anything is timed)
  unrescaled   hexl_hks_multiply_sum_relinearize, the fused call without the rescale, for the share the merged mod-down has
Operands and keys are uniform words (hexl_sample): the time of these calls does not depend on them. Every figure is the median of
`iters` calls, taken three times (`repeats`) with the routes alternating, so the spread is on record; `fused_over_three_call` < 1 means
the fused call is FASTER. Transform counts are the formulas of DESIGN.md 4.6.13. No ratio is promised. Writes and prints one JSON
document."""
import json
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]
import torch
import hexl_fpga_amd as hx
import orc

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "hks_multiply_rate.json"
N, L, ALPHA, N_P, BATCH, REPEATS = 16384, 12, 4, 4, 256, 3
K = L + N_P
LEVELS, TERMS = (12, 6), (1, 4)
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
moduli = orc.primes(K, 51, N)
plan = hx.KeySwitchPlan(ctx, N, L, K, K, 2, moduli, [pow(int(moduli[-1]), -1, int(q)) for q in moduli[:-1]] + [1])
hks = hx.HybridKeySwitch(plan, ALPHA)
dnum = -(-L // ALPHA)
hks.set_keys_device(uniform(plan, 2 * dnum, K, 1))
rows = []
for l in LEVELS:
    a = [uniform(plan, 2 * BATCH, l, 10 + t) for t in range(max(TERMS))]
    b = [uniform(plan, 2 * BATCH, l, 20 + t) for t in range(max(TERMS))]
    ct3 = torch.empty(BATCH * 3 * l * N, dtype=torch.int64, device=dev)
    ct2 = torch.empty(BATCH * 2 * l * N, dtype=torch.int64, device=dev)
    out = torch.empty(BATCH * 2 * (l - 1) * N, dtype=torch.int64, device=dev)
    dl = -(-l // ALPHA)
    digits = [min(ALPHA, l - d * ALPHA) for d in range(dl)]
    up_mac = l + sum(l + N_P - g for g in digits)                 # steps 1-2: the inverse and forward transforms of the mod-up
    for T in TERMS:
        def fused():
            hks.multiply_sum_rescale(out, a[:T], b[:T], BATCH, l)

        def three_call():
            plan.ct_tensor_sum(ct3, a[:T], b[:T], BATCH, l)
            hks.relinearize(ct2, ct3, BATCH, l)
            plan.rescale(out, ct2, BATCH, l, 2)

        def two_call():
            plan.ct_tensor_sum(ct3, a[:T], b[:T], BATCH, l)
            hks.relinearize_rescale(out, ct3, BATCH, l)

        def unrescaled():
            hks.multiply_sum_relinearize(ct2, a[:T], b[:T], BATCH, l)

        fused()
        first = out.clone()
        two_call()
        torch.cuda.synchronize()
        assert torch.equal(first, out), f"l = {l}, T = {T}: the fused call and its composition differ"
        del first
        routes = {"fused": fused, "three_call": three_call, "two_call": two_call, "unrescaled": unrescaled}
        ms = {k: [] for k in routes}
        for _ in range(REPEATS):
            for k, fn in routes.items():
                ms[k].append(timed(fn))
        rows.append({"n_limbs": l, "terms": T, "batch": BATCH, "ms": ms,
                     "products_per_s": {k: [BATCH / m * 1e3 for m in v] for k, v in ms.items()},
                     "fused_over_three_call": [f / t for f, t in zip(ms["fused"], ms["three_call"])],
                     "transforms_per_instance": {"fused": up_mac + 2 * N_P + 2 * l, "three_call": up_mac + 2 * N_P + 4 * l,
                                                 "mod_down_only": {"fused": 2 * N_P + 2 * l, "three_call": 2 * N_P + 4 * l}}})
        print(json.dumps(rows[-1]), flush=True)
    del a, b, ct3, ct2, out
    torch.cuda.empty_cache()
result = {"device": ctx.describe(), "iters": ITERS, "repeats": REPEATS, "n": N, "L": L, "alpha": ALPHA, "n_p": N_P, "K": K, "moduli_bits": 51,
          "mul_scratch_bytes": hks.mul_scratch_bytes(BATCH), "scratch_bytes": hks.scratch_bytes(BATCH), "rows": rows}
hks.close()
plan.close()
ctx.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
