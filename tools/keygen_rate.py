#!/usr/bin/env python3
"""keygen_rate.py [iters = 10] [out = profiles/keygen_rate.json] -- what keying ONE keyswitch plan costs, at N = 16384 on the headline
chain (K = 8, GeneratePrimes(8, 51, N), L = 7), relinearisation key, the shape of tools/rlwe_rate.py:
  (a) the host route: hexl_multiply_plain (s^2), L hexl_ct_lincomb (the plaintexts), one key-shaped hexl_rlwe_encrypt, ctx.sync(), the
      download of [L][2][K][N] words, hexl_ks_set_keys -- WALL CLOCK, since it synchronises and runs a host loop
  (b) a key that lives on the host: its upload from pinned memory + hexl_ks_set_keys_device -- wall clock to completion, and the device
      time of the install kernel alone
  (c) hexl_ks_gen_keys -- device events on the context's stream, and wall clock to completion
The three are checked against each other first: the same keyswitch output, word for word. Bytes of (c): the key kernel reads e and s
once per key row and s' in L rows, and writes c0 and a once per copy (three copies at N = 16384); the minimum the issue of this tool
counts re-reads e, s and s' for every copy. The error's pass through the encode scratch is listed separately.
Every figure is the median of `iters` calls, taken three times (`repeats`) with the routes alternating. Writes and prints one JSON
document."""
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
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "keygen_rate.json"
N, L, K, REPEATS, COPIES = 16384, 7, 8, 3, 3
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


def events(fn, iters=ITERS, warmup=2):
    """median milliseconds per call between device events"""
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
    return median(ms)


ctx = hx.Context(0)
moduli = orc.primes(K, 51, N)
case = KsCase(orc, N, L, K, seed=3, moduli=moduli)
qs = [int(q) for q in moduli]
P = qs[K - 1]
plans = [hx.KeySwitchPlan(ctx, N, L, K, K, 2, case.moduli, case.modswitch) for _ in range(3)]
pa, pb, pc = plans
secret = torch.empty(K * N, dtype=torch.int64, device=dev)
pa.sample(secret, hx.SAMPLE_TERNARY, 1, K, seed=SEED, stream=0)
s2 = torch.empty(K * N, dtype=torch.int64, device=dev)
pts = torch.empty(L * K * N, dtype=torch.int64, device=dev)
key = torch.empty(L * 2 * K * N, dtype=torch.int64, device=dev)
weights = [[[P % qs[i] if i == d else 0 for i in range(K)]] for d in range(L)]


def host_route():
    pa.multiply_plain(s2, secret, secret, 1, 1, K, 1)
    for d in range(L):
        pa.ct_lincomb(pts[d * K * N:(d + 1) * K * N], [s2], 1, 1, K, weights=weights[d])
    pa.rlwe_encrypt(key, secret, L, K, pt=pts, pt_batch=L, seed=SEED, stream=STREAM)
    ctx.sync()
    pa.set_keys(list(hx.to_u64(key).reshape(L, 2 * K * N)))


host_route()
host_key = torch.empty(L * 2 * K * N, dtype=torch.int64).pin_memory()
host_key.copy_(key)
landed = torch.empty_like(key)


def upload_and_install():
    landed.copy_(host_key, non_blocking=True)
    pb.set_keys_device(landed)


def install():
    pb.set_keys_device(landed)


def generate():
    pc.gen_relin_keys(secret, seed=SEED, stream=STREAM)


# word for word before any timing: one keyswitch on each of the three copies of the keys (1: lone path, 16: (b, d)-major, 64: slot-major)
upload_and_install()
generate()
for nb in (1, 16, 64):
    t = torch.empty(nb * L * N, dtype=torch.int64, device=dev)
    pa.sample(t, hx.SAMPLE_UNIFORM, nb, L, seed=SEED, stream=5)
    r0 = torch.empty(nb * 2 * L * N, dtype=torch.int64, device=dev)
    pa.sample(r0, hx.SAMPLE_UNIFORM, 2 * nb, L, seed=SEED, stream=6)
    outs = []
    for p in plans:
        r = r0.clone()
        p.keyswitch(r, t, nb)
        outs.append(r)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), f"the three routes leave different keys (batch {nb})"

rows = {k: [] for k in ("a_host_route_wall_ms", "b_upload_and_install_wall_ms", "b_install_kernel_device_ms", "c_generate_device_ms",
                        "c_generate_wall_ms")}
for _ in range(REPEATS):
    rows["a_host_route_wall_ms"].append(wall(host_route))
    rows["b_upload_and_install_wall_ms"].append(wall(upload_and_install))
    rows["b_install_kernel_device_ms"].append(events(install))
    rows["c_generate_device_ms"].append(events(generate))
    rows["c_generate_wall_ms"].append(wall(generate))
poly = N * 8
key_rows = L * (L + 1)
bytes_c = {"written_per_copy": key_rows * 2 * poly, "copies": COPIES,
           "read_by_the_key_kernel": key_rows * 2 * poly + L * poly,                                 # e and s per row, s' in L rows (L1/L2 serve the gather)
           "error_pass_through_scratch": 2 * L * poly + L * K * poly,                                # coefficients written and read, words written
           "minimum_of_the_issue": COPIES * (key_rows * 2 * poly + key_rows * 2 * poly + L * poly)}   # per copy: one write, e + s + s' read
bytes_c["moved_by_the_key_kernel"] = bytes_c["read_by_the_key_kernel"] + COPIES * bytes_c["written_per_copy"]
result = {"device": ctx.describe(), "iters": ITERS, "repeats": REPEATS, "n": N, "L": L, "K": K, "key_bytes_host_layout": L * 2 * K * poly,
          "rows": rows, "c_over_a": [c / a for c, a in zip(rows["c_generate_device_ms"], rows["a_host_route_wall_ms"])],
          "b_over_a": [b / a for b, a in zip(rows["b_upload_and_install_wall_ms"], rows["a_host_route_wall_ms"])],
          "bytes_c": bytes_c,
          "c_TBps_of_bytes_moved": [(bytes_c["moved_by_the_key_kernel"] + bytes_c["error_pass_through_scratch"]) / m * 1e-9
                                    for m in rows["c_generate_device_ms"]]}
for p in plans:
    p.close()
ctx.close()
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
