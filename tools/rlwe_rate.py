#!/usr/bin/env python3
"""rlwe_rate.py [iters = 10] [out = profiles/rlwe_rate.json] -- device rate of hexl_sample / hexl_rlwe_encrypt / hexl_rlwe_decrypt after
warm-up, timed with device events on the context's stream (the shape of tools/ct_lincomb_rate.py), at N = 16384 on the headline chain
(K = 8, GeneratePrimes(8, 51, N)), L = 7 limbs, batch 2048:
  (a) sample_uniform / sample_ternary / sample_cbd21 / encrypt / decrypt in TB/s of the bytes each MUST move: the output written once
      for a sampler ([batch][L][N] words), plaintext read + ciphertext written for encrypt (3 polynomials per instance; the secret is
      one polynomial for all), ciphertext read + result written for decrypt (3). The passes the small kinds and the error of an
      encryption make through the plan's scratch are the call's own business and are not counted: the figure is what the caller gets.
  (b) the fused encrypt against its own composition in the same process: hexl_sample(UNIFORM), hexl_sample(CBD21), hexl_multiply_plain,
      hexl_ct_lincomb (compared word for word first)
  (c) what a caller without the sampler pays instead: one H2D copy of the same [batch][2][L][N] words from pinned host memory
Every figure is the median of `iters` calls, taken three times (`repeats`) with the routes alternating, so the spread is on record.
Writes and prints one JSON document."""
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
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "rlwe_rate.json"
N, L, K, BATCH, REPEATS = 16384, 7, 8, 2048, 3
SEED, STREAM = bytes(range(32)), 1
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


ctx = hx.Context(0)
moduli = orc.primes(K, 51, N)
case = KsCase(orc, N, L, K, seed=3, moduli=moduli)
plan = hx.KeySwitchPlan(ctx, N, L, K, K, 2, case.moduli, case.modswitch)
qs = [int(q) for q in moduli[:L]]
poly_bytes = BATCH * L * N * 8                                     # one polynomial per instance at L limbs
words = BATCH * L * N
secret = torch.empty(K * N, dtype=torch.int64, device=dev)
plan.sample(secret, hx.SAMPLE_TERNARY, 1, K, seed=SEED, stream=0)
pt = torch.empty(words, dtype=torch.int64, device=dev)
plan.sample(pt, hx.SAMPLE_UNIFORM, BATCH, L, seed=SEED, stream=2)  # any words below their moduli serve as plaintexts
ct = torch.empty(2 * words, dtype=torch.int64, device=dev)
a, e, prod, c0, dec = (torch.empty(words, dtype=torch.int64, device=dev) for _ in range(5))
minus = [[1] * L, [q - 1 for q in qs]]


def sample(kind, out=a):
    plan.sample(out, kind, BATCH, L, seed=SEED, stream=STREAM)


def encrypt():
    plan.rlwe_encrypt(ct, secret, BATCH, L, pt=pt, pt_batch=BATCH, seed=SEED, stream=STREAM)


def composition():
    plan.sample(a, hx.SAMPLE_UNIFORM, BATCH, L, seed=SEED, stream=STREAM)
    plan.sample(e, hx.SAMPLE_CBD21, BATCH, L, seed=SEED, stream=STREAM)
    plan.multiply_plain(prod, a, secret, BATCH, 1, L, 1)
    plan.ct_lincomb(c0, [e, prod], BATCH, 1, L, weights=minus, pt=pt, pt_batch=BATCH)


def decrypt():
    plan.rlwe_decrypt(dec, ct, secret, BATCH, 2, L)


# word for word before any timing: the fused call is its composition, and decrypt(encrypt(pt)) - pt is the sampled error
encrypt()
composition()
decrypt()
plan.ct_lincomb(prod, [dec, pt], BATCH, 1, L, weights=minus)
torch.cuda.synchronize()
fused = ct.view(BATCH, 2, L * N)
assert torch.equal(fused[:, 0].reshape(-1), c0) and torch.equal(fused[:, 1].reshape(-1), a), "the fused encrypt and its composition differ"
assert torch.equal(prod, e), "decrypt(encrypt(pt)) - pt is not the error"

host = torch.empty(2 * words, dtype=torch.int64).pin_memory()
host.copy_(ct)
land = torch.empty_like(ct)
routes = {
    "sample_uniform": (lambda: sample(hx.SAMPLE_UNIFORM), poly_bytes),
    "sample_ternary": (lambda: sample(hx.SAMPLE_TERNARY), poly_bytes),
    "sample_cbd21": (lambda: sample(hx.SAMPLE_CBD21), poly_bytes),
    "encrypt": (encrypt, 3 * poly_bytes),
    "encrypt_composition": (composition, 3 * poly_bytes),
    "decrypt": (decrypt, 3 * poly_bytes),
    "h2d_copy_of_the_ciphertexts": (lambda: land.copy_(host, non_blocking=True), 2 * poly_bytes),
}
ms = {k: [] for k in routes}
for _ in range(REPEATS):
    for k, (fn, _) in routes.items():
        ms[k].append(timed(fn))
rows = {k: {"bytes_min": routes[k][1], "ms": v, "TBps_of_bytes_min": [routes[k][1] / m * 1e-9 for m in v]} for k, v in ms.items()}
copy_ms = [timed(lambda: c0.copy_(prod)) for _ in range(REPEATS)]
result = {"device": ctx.describe(), "iters": ITERS, "repeats": REPEATS, "n": N, "L": L, "K": K, "batch": BATCH,
          "moduli_bits": [q.bit_length() for q in qs], "polynomial_bytes_per_batch": poly_bytes, "rows": rows,
          "composition_over_fused": [c / f for c, f in zip(ms["encrypt_composition"], ms["encrypt"])],
          "h2d_over_fused": [c / f for c, f in zip(ms["h2d_copy_of_the_ciphertexts"], ms["encrypt"])],
          "torch_copy": {"bytes_read_plus_written": 2 * poly_bytes, "ms": copy_ms, "TBps": [2 * poly_bytes / m * 1e-9 for m in copy_ms]}}
plan.close()
ctx.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
