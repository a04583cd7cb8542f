#!/usr/bin/env python3
"""ckks_encode_rate.py [iters = 10] [output = profiles/ckks_encode_rate.json] -- device rates of hexl_ckks_encode and hexl_ckks_decode
after warm-up, timed with device events on the context's stream (tools/ckks_ops_rate.py's method), at N = 16384 on the headline chain
(GeneratePrimes(8, 51, N)) with n_limbs = 8 and n_limbs = 2, each beside what it is built from, measured in the same run at the same
count and n_limbs:
  encode/s     next to hexl_rns_ntt_fwd (the same transforms without the FFT and the scratch traffic) and hexl_rns_from_f64
  decode/s     next to hexl_rns_ntt_inv and hexl_rns_to_f64
Writes one JSON document and prints it."""
import json
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]
import torch
import hexl_fpga_amd as hx
import orc
from ks_util import KsCase

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "ckks_encode_rate.json"
N, K, COUNT, SCALE = 16384, 8, 1024, 2.0 ** 40
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


def rows_for(plan, n_limbs):
    g = torch.Generator(device=dev).manual_seed(n_limbs)
    slots = torch.rand((COUNT, N // 2, 2), dtype=torch.float64, device=dev, generator=g) * 2 - 1
    words = torch.empty(COUNT * n_limbs * N, dtype=torch.int64, device=dev)
    other = torch.empty_like(words)
    back = torch.empty_like(slots)
    coeffs = torch.empty((COUNT, N), dtype=torch.float64, device=dev)
    rate = lambda ms: {"ms": ms, "per_s": COUNT / ms * 1e3}
    row = {"n": N, "n_limbs": n_limbs, "count": COUNT, "scale_log2": 40}
    row["ckks_encode"] = rate(timed(lambda: plan.ckks_encode(words, slots, COUNT, n_limbs, SCALE)))
    row["ckks_decode"] = rate(timed(lambda: plan.ckks_decode(back, words, COUNT, n_limbs, SCALE)))
    row["round_trip_max_abs_error"] = float((back - slots).abs().max())
    row["rns_to_f64"] = rate(timed(lambda: plan.rns_to_f64(coeffs, words, COUNT, n_limbs)))
    row["rns_from_f64"] = rate(timed(lambda: plan.rns_from_f64(other, coeffs, COUNT, n_limbs)))
    row["from_f64_of_to_f64_is_identity"] = bool(torch.equal(other, words))
    row["rns_ntt_inv"] = rate(timed(lambda: plan.rns_ntt_inv(other, words, COUNT, n_limbs)))
    row["rns_ntt_fwd"] = rate(timed(lambda: plan.rns_ntt_fwd(other, other, COUNT, n_limbs)))
    row["encode_over_rns_ntt_fwd"] = row["rns_ntt_fwd"]["ms"] / row["ckks_encode"]["ms"]
    row["decode_over_rns_ntt_inv"] = row["rns_ntt_inv"]["ms"] / row["ckks_decode"]["ms"]
    # what crosses the bus per diagonal instead of the encoded rows
    row["slot_bytes_per_instance"], row["word_bytes_per_instance"] = N // 2 * 16, n_limbs * N * 8
    return row


ctx = hx.Context(0)
case = KsCase(orc, N, K - 1, K, seed=3, moduli=orc.primes(K, 51, N))
plan = hx.KeySwitchPlan(ctx, N, K - 1, K, K, 2, case.moduli, case.modswitch)
result = {"device": ctx.describe(), "iters": ITERS, "rows": [rows_for(plan, 8), rows_for(plan, 2)]}
assert plan.range_check(), "the timed inputs raised the range flag"
plan.close()
ctx.close()
text = json.dumps(result, indent=1)
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(text + "\n")
print(text)
