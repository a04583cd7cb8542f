#!/usr/bin/env python3
"""ct_lincomb_rate.py [iters = 10] [out = profiles/ct_lincomb_rate.json] -- device rate of hexl_ct_lincomb after warm-up, timed with device
events on the context's stream (the shape of tools/rns_ops_rate.py), at N = 16384 on the headline chain (L = 7, K = 8,
GeneratePrimes(8, 51, N)), batch 2048 x 2 components, for sums of T = 1, 2, 4, 8 ciphertexts with uniform weights:
  one_call       one hexl_ct_lincomb over T distinct buffers
  composition    the only route the C-ABI had before it, in the same process on the same buffers: T calls of hexl_multiply_plain with a
                 plaintext whose words are all w[t][i] (pt_batch 1) -- the first writes, the others accumulate
  one_call_null  the same sum with NULL weights (every weight 1: the path without the multiply)
Both routes are reported in TB/s of the traffic the SUM needs at least -- T terms read once, the output written once: (T + 1) x the
ciphertext bytes -- so the two figures compare directly; `ratio` = composition time / one-call time, against (3T - 1) / (T + 1) by pass
count (the composition reads a term and writes the output in its first call, and reads a term, reads and writes the output in each of
the others). A torch copy of one ciphertext is the ceiling on record. Every figure is the median of `iters` calls, taken three times
(`repeats`) with the routes alternating, so the spread is on record. Writes and prints one JSON document."""
import json
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]
import numpy as np
import torch
import hexl_fpga_amd as hx
import orc
from ks_util import KsCase

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "ct_lincomb_rate.json"
N, L, K, BATCH, NCOMP, REPEATS = 16384, 7, 8, 2048, 2, 3
TERMS = (1, 2, 4, 8)
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
    """[reps][len(moduli)][N] words below their limb's modulus"""
    g = torch.Generator(device=dev).manual_seed(seed)
    one = torch.stack([torch.randint(0, int(q), (N,), dtype=torch.int64, device=dev, generator=g) for q in moduli])
    return one.repeat(reps, 1, 1).reshape(-1)


ctx = hx.Context(0)
moduli = orc.primes(K, 51, N)
case = KsCase(orc, N, L, K, seed=3, moduli=moduli)
plan = hx.KeySwitchPlan(ctx, N, L, K, K, 2, case.moduli, case.modswitch)
qs = [int(q) for q in moduli[:L]]
ct_bytes = BATCH * NCOMP * L * N * 8
terms = [residues(qs * NCOMP, BATCH, 100 + t) for t in range(max(TERMS))]
out = torch.empty_like(terms[0])
rng = np.random.default_rng(7)
weights = [[int(rng.integers(2, q - 1)) for q in qs] for _ in range(max(TERMS))]
pts = [hx.as_i64(np.array([np.full(N, w[i], dtype=np.uint64) for i in range(L)]).reshape(-1)).to(dev) for w in weights]


def one_call(T, w):
    plan.ct_lincomb(out, terms[:T], BATCH, NCOMP, L, weights=None if w is None else w[:T])


def composition(T):
    for t in range(T):
        plan.multiply_plain(out, terms[t], pts[t], BATCH, NCOMP, L, 1, accumulate=t > 0)


rows = []
for T in TERMS:
    # the two routes give the same words
    one_call(T, weights)
    a = out.clone()
    composition(T)
    torch.cuda.synchronize()
    assert torch.equal(a, out), f"T = {T}: the one call and the composition differ"
    del a
    nbytes = (T + 1) * ct_bytes
    ms = {"one_call": [], "composition": [], "one_call_null": []}
    for _ in range(REPEATS):
        ms["one_call"].append(timed(lambda: one_call(T, weights)))
        ms["composition"].append(timed(lambda: composition(T)))
        ms["one_call_null"].append(timed(lambda: one_call(T, None)))
    row = {"terms": T, "bytes_min": nbytes, "passes_one_call": T + 1, "passes_composition": 3 * T - 1,
           "ratio_by_pass_count": (3 * T - 1) / (T + 1)}
    for key, v in ms.items():
        row[key] = {"ms": v, "TBps_of_bytes_min": [nbytes / m * 1e-9 for m in v]}
    row["ratio"] = [c / o for c, o in zip(ms["composition"], ms["one_call"])]
    rows.append(row)
copy_ms = [timed(lambda: out.copy_(terms[0])) for _ in range(REPEATS)]
result = {"device": ctx.describe(), "iters": ITERS, "repeats": REPEATS, "n": N, "L": L, "K": K, "batch": BATCH, "components": NCOMP,
          "moduli_bits": [q.bit_length() for q in qs], "ciphertext_bytes": ct_bytes, "rows": rows,
          "torch_copy": {"bytes_read_plus_written": 2 * ct_bytes, "ms": copy_ms, "TBps": [2 * ct_bytes / m * 1e-9 for m in copy_ms]}}
plan.close()
ctx.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
