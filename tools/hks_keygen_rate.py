#!/usr/bin/env python3
"""hks_keygen_rate.py [iters = 10] [out = profiles/hks_keygen_rate.json] -- what keying a SET of hybrid objects costs, at N = 16384,
L = 12, alpha = 4, K = 16 (dnum = 3; GeneratePrimes(16, 51, N)), Galois keys for 5^1 ... 5^R, R = 1, 7, 15 (15: an 8 x 8 BSGS layer):
  (a) the wrapper route, per key: hexl_apply_galois on the secret, KeySwitchPlan.gen_hybrid_key (dnum hexl_ct_lincomb + one key-shaped
      hexl_rlwe_encrypt into a [dnum][2][K][N] word buffer), hexl_hks_set_keys_device
  (b) ONE hexl_hks_keygen call for the R objects
Both are WALL CLOCK with the host's share included: the stream is synchronised before the clock starts and before it stops. The two
routes run in the same process on the same objects' shapes and are checked against each other first: hexl_hks_export_keys of every
object, word for word. Every figure is the median of `iters` calls, taken three times (`repeats`) with the routes alternating. The
byte counts are counts from the code (units of W = dnum K N words per key), not measurements. Writes and prints one JSON document."""
import json
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]
import torch
import hexl_fpga_amd as hx
import orc
from ks_util import KsCase

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "hks_keygen_rate.json"
N, L, ALPHA, K, REPEATS = 16384, 12, 4, 16, 3
COUNTS = (1, 7, 15)
SEED, STREAM = bytes(range(32)), 1
dev = torch.device("cuda:0")


def median(v):
    v = sorted(v)
    return 0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2])


def wall(fn, iters=ITERS, warmup=2):
    """median milliseconds per call, host clock, the device idle before and after"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return median(ms)


ctx = hx.Context(0)
case = KsCase(orc, N, L, K, seed=3, moduli=orc.primes(K, 51, N))
plan = hx.KeySwitchPlan(ctx, N, L, K, K, 2, case.moduli, case.modswitch)
DNUM = -(-L // ALPHA)
R_MAX = max(COUNTS)
elts = [pow(5, r + 1, 2 * N) for r in range(R_MAX)]
wrapped = [hx.HybridKeySwitch(plan, ALPHA) for _ in range(R_MAX)]
fused = [hx.HybridKeySwitch(plan, ALPHA) for _ in range(R_MAX)]
secret = torch.empty(K * N, dtype=torch.int64, device=dev)
plan.sample(secret, hx.SAMPLE_TERNARY, 1, K, seed=SEED, stream=0)
s_g = torch.empty(K * N, dtype=torch.int64, device=dev)
words = torch.empty(DNUM * 2 * K * N, dtype=torch.int64, device=dev)


def wrapper_route(count):
    for r in range(count):
        ctx.apply_galois(s_g, secret, K, N, elts[r])
        plan.gen_hybrid_key(words, secret, ALPHA, s_g, seed=SEED, stream=STREAM, first=r * DNUM)
        wrapped[r].set_keys_device(words)


def fused_route(count):
    hx.hks_keygen(fused[:count], secret, [hx.KEY_FROM_GALOIS] * count, galois_elts=elts[:count], seed=SEED, stream=STREAM, first=0)


# word for word before any timing
wrapper_route(R_MAX)
fused_route(R_MAX)
a, b = torch.empty_like(words), torch.empty_like(words)
for r in range(R_MAX):
    wrapped[r].export_keys(a)
    fused[r].export_keys(b)
    torch.cuda.synchronize()
    assert torch.equal(a, b), f"the two routes leave different keys (key {r})"

rows = {}
for count in COUNTS:
    w, f = [], []
    for _ in range(REPEATS):
        w.append(wall(lambda: wrapper_route(count)))
        f.append(wall(lambda: fused_route(count)))
    rows[f"{count}_keys"] = {"wrapper_route_wall_ms": w, "hks_keygen_wall_ms": f, "keygen_over_wrapper": [y / x for x, y in zip(w, f)],
                             "wrapper_over_keygen_median": median(w) / median(f)}
W = DNUM * K * N * 8
result = {"device": ctx.describe(), "what": "one run, one machine; wall clock with the host's share, stream synchronised at both ends",
          "iters": ITERS, "repeats": REPEATS, "n": N, "L": L, "alpha": ALPHA, "K": K, "dnum": DNUM, "key_bytes_installed": 2 * W, "rows": rows,
          "counted_not_measured": {"W_bytes": W, "wrapper_route_W": {"lincomb": 2, "error": 1, "encrypt": 4, "install": 4},
                                   "hks_keygen_W": {"error_write": 1, "error_read": 1, "key_store": 2},
                                   "wrapper_route_launches_per_key": 5 + DNUM, "hks_keygen_launches_per_call": 3}}
for h in wrapped + fused:
    h.close()
plan.close()
ctx.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
