#!/usr/bin/env python3
"""pk_rate.py [iters = 10] [out = profiles/pk_encrypt_rate.json] -- device rate of hexl_pk_encrypt after warm-up, timed with device
events on the context's stream (the shape of tools/rlwe_rate.py), at N = 16384 on the headline chain (K = 8, GeneratePrimes(8, 51, N)),
L = 7 limbs, batch 2048, a key kept at K limbs:
  (a) the fused call in TB/s of the bytes it MUST move: the plaintext read and the two components written (3 polynomials per
      instance; the key is two polynomials for all). The passes the mask and the errors make through the plan's scratch are the call's
      own business and are not counted: the figure is what the caller gets.
  (b) the fused call against its normative composition in the same process: hexl_sample(TERNARY), hexl_sample(CBD21), the key's first L
      limbs replicated once per instance (a strided device copy -- part of what a caller without the entry point has to do),
      hexl_multiply_plain, hexl_ct_lincomb (compared word for word first)
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
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "pk_encrypt_rate.json"
N, L, K, BATCH, REPEATS = 16384, 7, 8, 2048, 3
SEED, STREAM, FIRST = bytes(range(32)), 1, 0
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
poly_bytes = BATCH * L * N * 8                                     # one polynomial per instance at L limbs
words = BATCH * L * N
secret = torch.empty(K * N, dtype=torch.int64, device=dev)
plan.sample(secret, hx.SAMPLE_TERNARY, 1, K, seed=SEED, stream=0)
pk = torch.empty(2 * K * N, dtype=torch.int64, device=dev)
plan.gen_public_key(pk, secret, seed=SEED, stream=3)
pt = torch.empty(words, dtype=torch.int64, device=dev)
plan.sample(pt, hx.SAMPLE_UNIFORM, BATCH, L, seed=SEED, stream=2)  # any words below their moduli serve as plaintexts
ct, E, rep, T, composed = (torch.empty(2 * words, dtype=torch.int64, device=dev) for _ in range(5))
U = torch.empty(words, dtype=torch.int64, device=dev)
key_view = pk.view(1, 2, K, N)[:, :, :L]


def fused():
    plan.pk_encrypt(ct, pk, BATCH, L, pk_limbs=K, pt=pt, pt_batch=BATCH, seed=SEED, stream=STREAM, first=FIRST)


def composition():
    plan.sample(U, hx.SAMPLE_TERNARY, BATCH, L, seed=SEED, stream=STREAM, first=FIRST)
    plan.sample(E, hx.SAMPLE_CBD21, 2 * BATCH, L, seed=SEED, stream=STREAM, first=2 * FIRST)
    rep.view(BATCH, 2, L, N).copy_(key_view.expand(BATCH, 2, L, N))
    plan.multiply_plain(T, rep, U, BATCH, 2, L, BATCH)
    plan.ct_lincomb(composed, [T, E], BATCH, 2, L, pt=pt, pt_batch=BATCH)


# word for word before any timing: the fused call is its composition, and it decrypts to the plaintext plus a small noise
fused()
composition()
dec = torch.empty(words, dtype=torch.int64, device=dev)
plan.rlwe_decrypt(dec, ct, secret, BATCH, 2, L)
torch.cuda.synchronize()
assert torch.equal(ct, composed), "the fused public-key encrypt and its composition differ"
assert not torch.equal(dec, pt), "no noise at all: the key is not a key"
del dec

routes = {"pk_encrypt": (fused, 3 * poly_bytes), "pk_encrypt_composition": (composition, 3 * poly_bytes)}
ms = {k: [] for k in routes}
for _ in range(REPEATS):
    for k, (fn, _) in routes.items():
        ms[k].append(timed(fn))
rows = {k: {"bytes_min": routes[k][1], "ms": v, "TBps_of_bytes_min": [routes[k][1] / m * 1e-9 for m in v]} for k, v in ms.items()}
copy_ms = [timed(lambda: U.copy_(pt)) for _ in range(REPEATS)]
result = {"device": ctx.describe(), "iters": ITERS, "repeats": REPEATS, "n": N, "L": L, "K": K, "pk_limbs": K, "batch": BATCH,
          "moduli_bits": [int(q).bit_length() for q in moduli[:L]], "polynomial_bytes_per_batch": poly_bytes, "rows": rows,
          "composition_over_fused": [c / f for c, f in zip(ms["pk_encrypt_composition"], ms["pk_encrypt"])],
          "torch_copy": {"bytes_read_plus_written": 2 * poly_bytes, "ms": copy_ms, "TBps": [2 * poly_bytes / m * 1e-9 for m in copy_ms]}}
plan.close()
ctx.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
