#!/usr/bin/env python3
"""tensor_relin_rate.py [iters = 5] [out = profiles/tensor_relin_rate.json] -- device time of a relinearised sum of T ciphertext products
after warm-up, timed with device events on the context's stream (the shape of tools/ct_lincomb_rate.py), at N = 16384 on the headline
chain (L = 7, K = 8, GeneratePrimes(8, 51, N)), batch 256, for T = 2, 4, 8:
  fused         one hexl_multiply_sum_relinearize: one tensor kernel and ONE key switch per slice
  per_pair      what a caller wrote before it, in the same process on the same buffers: T x hexl_multiply_relinearize into temporaries,
                then one hexl_ct_lincomb over the T results (not word-identical to `fused`: T roundings by the special prime against
                one; both decrypt to the same plaintext)
  composition   hexl_ct_tensor_sum then hexl_relinearize (word for word `fused`, asserted here before anything is timed)
  one_pair      one hexl_multiply_relinearize, the cost the fused call should approach per output as T grows
and hexl_ct_tensor_sum alone at batch 1024 against the bytes it must move, (4 T + 3) polynomial passes per limb, with a torch copy as the
ceiling on record. Every figure is the median of `iters` calls, taken three times (`repeats`) with the routes alternating, so the spread
is on record. Writes and prints one JSON document."""
import json
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]
import torch
import hexl_fpga_amd as hx
import orc
from ks_util import KsCase

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "tensor_relin_rate.json"
N, L, K, BATCH, TENSOR_BATCH, REPEATS = 16384, 7, 8, 256, 1024, 3
TERMS = (2, 4, 8)
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


def residues(moduli, reps, seed):
    """[reps][len(moduli)][N] words below their limb's modulus (one instance, repeated)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    one = torch.stack([torch.randint(0, int(q), (N,), dtype=torch.int64, device=dev, generator=g) for q in moduli])
    return one.repeat(reps, 1, 1).reshape(-1)


ctx = hx.Context(0)
moduli = orc.primes(K, 51, N)
case = KsCase(orc, N, L, K, seed=3, moduli=moduli)
plan = hx.KeySwitchPlan(ctx, N, L, K, K, 2, case.moduli, case.modswitch)
plan.set_keys(case.keys)
qs = [int(q) for q in moduli[:L]]
ct_bytes = BATCH * 2 * L * N * 8
a = [residues(qs * 2, BATCH, 100 + t) for t in range(max(TERMS))]
b = [residues(qs * 2, BATCH, 200 + t) for t in range(max(TERMS))]
out = torch.empty_like(a[0])
tmp = [torch.empty_like(a[0]) for _ in range(max(TERMS))]
ct3 = torch.empty(BATCH * 3 * L * N, dtype=torch.int64, device=dev)


def fused(T):
    plan.multiply_sum_relinearize(out, a[:T], b[:T], BATCH)


def per_pair(T):
    for t in range(T):
        plan.multiply_relinearize(tmp[t], a[t], b[t], BATCH)
    plan.ct_lincomb(out, tmp[:T], BATCH, 2, L)


def composition(T):
    plan.ct_tensor_sum(ct3, a[:T], b[:T], BATCH, L)
    plan.relinearize(out, ct3, BATCH)


rows = []
for T in TERMS:
    fused(T)
    first = out.clone()
    composition(T)
    torch.cuda.synchronize()
    assert torch.equal(first, out), f"T = {T}: the fused call and its composition differ"
    del first
    ms = {"fused": [], "per_pair": [], "composition": []}
    for _ in range(REPEATS):
        ms["fused"].append(timed(lambda: fused(T)))
        ms["per_pair"].append(timed(lambda: per_pair(T)))
        ms["composition"].append(timed(lambda: composition(T)))
    rows.append({"terms": T, "ms": ms, "per_pair_over_fused": [p / f for p, f in zip(ms["per_pair"], ms["fused"])],
                 "transforms_saved_per_instance": (T - 1) * (L * L + 3 * L + 2)})
one_pair = [timed(lambda: plan.multiply_relinearize(out, a[0], b[0], BATCH)) for _ in range(REPEATS)]
keyswitch = [timed(lambda: plan.keyswitch(out, ct3[:BATCH * L * N], BATCH)) for _ in range(REPEATS)]
assert plan.range_check()
del tmp, ct3, out

# the tensor kernel alone, against the bytes it must move
ta = [residues(qs * 2, TENSOR_BATCH, 300 + t) for t in range(max(TERMS))]
tb = [residues(qs * 2, TENSOR_BATCH, 400 + t) for t in range(max(TERMS))]
t3 = torch.empty(TENSOR_BATCH * 3 * L * N, dtype=torch.int64, device=dev)
poly_bytes = TENSOR_BATCH * L * N * 8
tensor_rows = []
for T in (1,) + TERMS:
    nbytes = (4 * T + 3) * poly_bytes
    ms = [timed(lambda: plan.ct_tensor_sum(t3, ta[:T], tb[:T], TENSOR_BATCH, L), iters=2 * ITERS) for _ in range(REPEATS)]
    tensor_rows.append({"terms": T, "bytes_min": nbytes, "passes": 4 * T + 3, "ms": ms, "TBps_of_bytes_min": [nbytes / m * 1e-9 for m in ms]})
copy_ms = [timed(lambda: t3[:2 * TENSOR_BATCH * L * N].copy_(ta[0]), iters=2 * ITERS) for _ in range(REPEATS)]
result = {"device": ctx.describe(), "iters": ITERS, "repeats": REPEATS, "n": N, "L": L, "K": K, "batch": BATCH,
          "moduli_bits": [q.bit_length() for q in qs], "ciphertext_bytes": ct_bytes, "rows": rows,
          "one_multiply_relinearize_ms": one_pair, "one_keyswitch_ms": keyswitch,
          "tensor_sum_alone": {"batch": TENSOR_BATCH, "rows": tensor_rows,
                               "torch_copy": {"bytes_read_plus_written": 4 * poly_bytes, "ms": copy_ms,
                                              "TBps": [4 * poly_bytes / m * 1e-9 for m in copy_ms]}}}
plan.close()
ctx.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
