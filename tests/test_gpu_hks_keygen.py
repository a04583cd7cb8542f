"""GPU: hexl_hks_keygen and hexl_hks_export_keys. Every generated key is read back with hexl_hks_export_keys and compared word for word,
every word of every row, against the device composition that defines it (plan.gen_hybrid_key -> hexl_hks_set_keys_device, s' by
hexl_multiply_plain / hexl_apply_galois) and, at the small rings, against tests/hks_keygen_model.py: n = 1024 (one 1024-word piece per
row) and n = 2048 (two) with L = 3, K = 5 and alpha = 1, 2 (a partial last digit), 3 (one digit), every kind, non-zero stream and first;
a set of four objects with alpha = 2, 2, 1, 3 in one call and split into two; a mixed-tier chain; n = 16384 and n = 32768; the errors in
several chunks of the encode scratch (a child process with HEXL_HKS_KEYGEN_CHUNK); the export round trip; re-keying an object in use
without a synchronisation, on the session's stream and on a non-blocking caller stream; every refusal on the device; and end to end at
l = L and l = L - 1: a generated relinearisation key under hexl_ct_tensor_sum -> hexl_hks_relinearize, and two generated Galois keys
under hexl_hks_linear_transform, decrypted within the bounds the existing hybrid tests use."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import hks_hoisted_model
import hks_keygen_model as km
from ckks_model import Limbs, apply_galois
from hks_model import Hks
from ks_util import KsCase, seal_chain

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG, HEXL_E_NOKEYS = -1, -2
SEED = bytes((37 * k + 11) & 0xFF for k in range(32))
POLY, SQUARE, GALOIS = km.FROM_POLY, km.FROM_SQUARE, km.FROM_GALOIS


def torch_():
    import torch
    return torch


def up(hx, dev, a):
    return hx.as_i64(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)).to(dev)


def minus_one(dev, words):
    return torch_().full((words,), -1, dtype=torch_().int64, device=dev)


class Env:
    """an FP64 plan with K > L, a ternary secret at K limbs and a uniform polynomial for KEY_FROM_POLY, all made on the device"""

    def __init__(self, hx, ctx, dev, orc, n, L, K, moduli):
        self.hx, self.ctx, self.dev, self.n, self.L, self.K = hx, ctx, dev, n, L, K
        case = KsCase(orc, n, L, K, moduli=moduli)
        self.qs = [int(q) for q in case.moduli]
        self.plan = hx.KeySwitchPlan(ctx, n, L, K, K, 2, case.moduli, case.modswitch)
        self.sec, self.poly = minus_one(dev, K * n), minus_one(dev, K * n)
        torch_().cuda.synchronize()                               # the fills ran on torch's stream, the context may be on another
        self.plan.sample(self.sec, hx.SAMPLE_TERNARY, 1, K, seed=SEED, stream=1)
        self.plan.sample(self.poly, hx.SAMPLE_UNIFORM, 1, K, seed=SEED, stream=9)
        self.objs = []

    def obj(self, alpha):
        self.objs.append(self.hx.HybridKeySwitch(self.plan, alpha))
        return self.objs[-1]

    def s_from(self, kind, g):
        """s' on the device by the routes the wrapper's callers use"""
        if kind == POLY:
            return self.poly
        out = minus_one(self.dev, self.K * self.n)
        if kind == SQUARE:
            self.plan.multiply_plain(out, self.sec, self.sec, 1, 1, self.K, 1)
        else:
            self.ctx.apply_galois(out, self.sec, self.K, self.n, g)
        return out

    def wrapper_words(self, alpha, kind, g, stream, first):
        """the wrapper composition: gen_hybrid_key's words, installed on an object of their own and exported -- what
        hexl_hks_set_keys_device leaves for them -- as a host array [dnum][2][K][n]"""
        dnum = -(-self.L // alpha)
        words = minus_one(self.dev, dnum * 2 * self.K * self.n)
        self.plan.gen_hybrid_key(words, self.sec, alpha, self.s_from(kind, g), seed=SEED, stream=stream, first=first)
        h = self.hx.HybridKeySwitch(self.plan, alpha)
        h.set_keys_device(words)
        out = minus_one(self.dev, words.numel())
        h.export_keys(out)
        self.ctx.sync()
        h.close()
        assert self.hx.to_u64(out).tobytes() == self.hx.to_u64(words).tobytes(), "the wrapper's words are canonical: the export returns them"
        return self.hx.to_u64(out)

    def exported(self, h):
        out = minus_one(self.dev, h.dnum * 2 * self.K * self.n)
        h.export_keys(out)
        self.ctx.sync()
        return self.hx.to_u64(out)

    def model_words(self, orc, alpha, kind, g, stream, first, lm=None):
        m = Hks(orc, self.n, self.L, self.K, alpha, self.qs, lm=lm)
        s = self.hx.to_u64(self.sec).reshape(self.K, self.n)
        poly = self.hx.to_u64(self.poly).reshape(self.K, self.n) if kind == POLY else None
        return km.key(m, SEED, stream, first, s, km.from_words(m, s, kind, g, poly))

    def close(self):
        for o in reversed(self.objs):
            o.close()
        self.plan.close()


def same_words(got, want, env, label):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, label
    bad = np.flatnonzero(got != want)
    if len(bad):
        row, j = divmod(int(bad[0]), env.n)
        dk, i = divmod(row, env.K)
        raise AssertionError(f"{label}: {len(bad)} of {got.size} words differ, the first at row d = {dk // 2}, component {dk % 2}, limb {i}, "
                             f"coefficient {j}: got {int(got[bad[0]])}, want {int(want[bad[0]])}")


def kinds_of(n):
    # (kind, Galois element, stream, first): a large stream number, first = 0 once and the last admissible first once
    return [(SQUARE, 4, 3, 5), (GALOIS, 5, 0xFEDCBA9876543210, 0), (GALOIS, 2 * n - 1, 4, (1 << 40) - 3), (POLY, 0, 2, 77)]


@pytest.mark.parametrize("alpha", [1, 2, 3])
@pytest.mark.parametrize("n", [1024, 2048])
def test_smallest_rings_every_kind(hx, ctx, dev, orc, n, alpha):
    L, K = 3, 5
    env = Env(hx, ctx, dev, orc, n, L, K, orc.primes(K, 51, n))
    sec_before, poly_before = env.sec.clone(), env.poly.clone()
    h = env.obj(alpha)
    lm = Limbs(orc, n, env.qs)
    for kind, g, stream, first in kinds_of(n):
        # what the kind does not use is ignored: an even element for the square, a stray polynomial for the Galois key
        h.gen_keys(env.sec, kind, galois_elt=g, from_poly=None if kind == SQUARE else env.poly, seed=SEED, stream=stream, first=first)
        got = env.exported(h)
        label = f"n = {n}, alpha = {alpha}, kind {kind}, g = {g}"
        same_words(got, env.wrapper_words(alpha, kind, g, stream, first), env, label + " against the wrapper composition")
        same_words(got, env.model_words(orc, alpha, kind, g, stream, first, lm), env, label + " against the model")
    assert torch_().equal(env.sec, sec_before) and torch_().equal(env.poly, poly_before), "an input was written"
    env.close()


SET = dict(alphas=[2, 2, 1, 3], kinds=[SQUARE, GALOIS, GALOIS, POLY], elts=[0, 5, 2047, 2], stream=6, first=1000)


def generate_set(hx, ctx, dev, orc):
    """the four-object set in ONE call -> (env, [exported words per object]); the chunking test's child process runs the same"""
    n, L, K = 1024, 3, 5
    env = Env(hx, ctx, dev, orc, n, L, K, orc.primes(K, 51, n))
    objs = [env.obj(a) for a in SET["alphas"]]
    raw = hx.hks_keygen(objs, env.sec, SET["kinds"], galois_elts=SET["elts"], from_polys=[None, None, None, env.poly], seed=SEED,
                        stream=SET["stream"], first=SET["first"])
    assert raw == SEED
    return env, objs, [env.exported(o) for o in objs]


def test_a_key_set_in_one_call(hx, ctx, dev, orc):
    env, objs, got = generate_set(hx, ctx, dev, orc)
    dnums = [o.dnum for o in objs]
    assert dnums == [2, 2, 3, 1]
    for r, o in enumerate(objs):
        first_r = SET["first"] + sum(dnums[:r])
        want = env.wrapper_words(SET["alphas"][r], SET["kinds"][r], SET["elts"][r], SET["stream"], first_r)
        same_words(got[r], want, env, f"key {r} of the set against its own wrapper result at first = {first_r}")
    # the same set in two calls on fresh objects, `first` advanced by the rows of the first call
    again = [env.obj(a) for a in SET["alphas"]]
    hx.hks_keygen(again[:2], env.sec, SET["kinds"][:2], galois_elts=SET["elts"][:2], seed=SEED, stream=SET["stream"], first=SET["first"])
    hx.hks_keygen(again[2:], env.sec, SET["kinds"][2:], galois_elts=SET["elts"][2:], from_polys=[None, env.poly], seed=SEED,
                  stream=SET["stream"], first=SET["first"] + sum(dnums[:2]))
    for r, o in enumerate(again):
        same_words(env.exported(o), got[r], env, f"key {r}: two calls against one")
    env.close()


def test_the_errors_in_several_chunks(hx, ctx, dev, orc, tmp_path):
    """HEXL_HKS_KEYGEN_CHUNK=3 (read once per process, so a child process): the 8 rows of the set go through the encode scratch as
    3 + 3 + 2, the chunks cutting through keys 1 and 2; this process runs them as one chunk (8 rows <= 4096 at n = 1024)"""
    env, objs, got = generate_set(hx, ctx, dev, orc)
    env.close()
    ref = tmp_path / "one_chunk.npz"
    np.savez(ref, **{f"key{r}": w for r, w in enumerate(got)})
    code = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch, hexl_fpga_amd as hx, orc
from test_gpu_hks_keygen import generate_set
dev = torch.device("cuda:0")
ctx = hx.Context(0)
env, objs, got = generate_set(hx, ctx, dev, orc)
want = np.load(%r)
for r, w in enumerate(got):
    assert np.array_equal(w, want["key%%d" %% r]), "key %%d differs from the one-chunk words" %% r
env.close()
print("CHUNKS OK")
''' % (str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests"), str(ref))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, HEXL_HKS_KEYGEN_CHUNK="3"))
    print(out.stdout[-1000:], out.stderr[-1500:])
    assert out.returncode == 0 and "CHUNKS OK" in out.stdout


def test_mixed_tier_chain(hx, ctx, dev, orc):
    """52, 30, 30, 40, 27-bit data limbs and two 27-bit special primes (L = 5, alpha = 2, K = 7): every limb on its own tier's constants"""
    n, L, K, alpha = 1024, 5, 7, 2
    env = Env(hx, ctx, dev, orc, n, L, K, seal_chain(orc, K, n))
    tiers, mixed = env.plan.tiers()
    assert mixed and tiers[0] == 0 and all(t != 0 for t in tiers[1:]), tiers
    h = env.obj(alpha)
    for kind, g, stream, first in ((GALOIS, 5, 8, 3), (SQUARE, 1, 8, 6)):
        h.gen_keys(env.sec, kind, galois_elt=g, seed=SEED, stream=stream, first=first)
        got = env.exported(h)
        same_words(got, env.wrapper_words(alpha, kind, g, stream, first), env, f"mixed tiers, kind {kind} against the wrapper composition")
        same_words(got, env.model_words(orc, alpha, kind, g, stream, first), env, f"mixed tiers, kind {kind} against the model")
    env.close()


@pytest.mark.parametrize("n", [16384, 32768])
def test_large_rings(hx, ctx, dev, orc, n):
    L, K, alpha = 3, 5, 2
    env = Env(hx, ctx, dev, orc, n, L, K, orc.primes(K, 51, n))
    h = env.obj(alpha)
    h.gen_galois_keys(env.sec, 5, seed=SEED, stream=2, first=9)
    same_words(env.exported(h), env.wrapper_words(alpha, GALOIS, 5, 2, 9), env, f"n = {n} against the wrapper composition")
    env.close()


def random_key_words(env, dnum, salt):
    """[dnum][2][K][n] full-range 64-bit words, most of them >= q, with rows of q - 1, q and 2^64 - 1 between"""
    rng = np.random.default_rng(500 + salt)
    w = rng.integers(0, 1 << 64, size=(dnum * 2 * env.K, env.n), dtype=np.uint64)
    for row in range(dnum * 2 * env.K):
        q = env.qs[row % env.K]
        if row % 4 == 1:
            w[row] = np.uint64([q - 1, q, 0xFFFFFFFFFFFFFFFF, 0][row // 4 % 4])
    return w


def test_export_round_trip(hx, ctx, dev, orc):
    torch = torch_()
    n, L, K, alpha = 1024, 3, 5, 2
    env = Env(hx, ctx, dev, orc, n, L, K, orc.primes(K, 51, n))
    a, b = env.obj(alpha), env.obj(alpha)
    out = minus_one(dev, a.dnum * 2 * K * n)
    with pytest.raises(hx.HexlError, match="status -2"):
        a.export_keys(out)
    ctx.sync()
    assert bool((out == -1).all()), "an export without keys wrote"
    words = random_key_words(env, a.dnum, 1)
    d_words = up(hx, dev, words)
    a.set_keys_device(d_words)
    a.export_keys(out)
    ctx.sync()
    want = np.stack([words[row] % np.uint64(env.qs[row % K]) for row in range(len(words))])
    same_words(hx.to_u64(out), want, env, "set_keys_device -> export against the words modulo q")
    assert np.array_equal(hx.to_u64(d_words), words.reshape(-1)), "the install's input was written"
    # export -> install on a second object: the same key switch, and the same export
    b.set_keys_device(out)
    rng = np.random.default_rng(3)
    t = up(hx, dev, np.concatenate([rng.integers(0, q, size=n, dtype=np.uint64) for q in env.qs[:L]]))
    ra, rb = torch.zeros(2 * L * n, dtype=torch.int64, device=dev), torch.zeros(2 * L * n, dtype=torch.int64, device=dev)
    a.keyswitch(ra, t, 1, L)
    b.keyswitch(rb, t, 1, L)
    ctx.sync()
    assert bool(ra.any()) and torch.equal(ra, rb), "the re-installed export switches differently"
    same_words(env.exported(b), want, env, "export -> install -> export")
    env.close()


def rekey_in_use(hx, own, dev, orc, env_ctx_sync):
    """generate (g = 5), rotate, generate (g = 2n - 1), rotate on ONE object with nothing waited for in between; the expected outputs come
    from two objects keyed once each with the same triples"""
    torch = torch_()
    n, L, K, alpha = 1024, 3, 5, 2
    env = Env(hx, own, dev, orc, n, L, K, orc.primes(K, 51, n))
    gs = [(5, 0), (2 * n - 1, 2)]                                 # (element, first): the second key draws the next dnum polynomials
    rng = np.random.default_rng(7)
    ct = up(hx, dev, np.concatenate([rng.integers(0, q, size=n, dtype=np.uint64) for _ in range(2) for q in env.qs[:L]]))
    outs = [minus_one(dev, 2 * L * n) for _ in range(4)]
    once = [env.obj(alpha) for _ in gs]
    used = env.obj(alpha)
    env_ctx_sync()                                                # the uploads and the samples above
    for (g, first), o, out in zip(gs, once, outs[2:]):
        o.gen_galois_keys(env.sec, g, seed=SEED, stream=4, first=first)
        o.rotate(out, ct, 1, L, g)
    env_ctx_sync()
    for (g, first), out in zip(gs, outs[:2]):
        used.gen_galois_keys(env.sec, g, seed=SEED, stream=4, first=first)
        used.rotate(out, ct, 1, L, g)
    env_ctx_sync()
    assert not torch.equal(outs[2], outs[3])
    assert torch.equal(outs[0], outs[2]), "the first rotation did not see the first key"
    assert torch.equal(outs[1], outs[3]), "the second rotation did not see the second key"
    env.close()


def test_rekey_in_use_without_a_synchronisation(hx, ctx, dev, orc):
    rekey_in_use(hx, ctx, dev, orc, ctx.sync)


def test_rekey_in_use_on_a_non_blocking_caller_stream(hx, dev, orc):
    torch = torch_()
    own = hx.Context(0, use_torch_stream=False)
    side = torch.cuda.Stream()
    own.set_stream(side.cuda_stream)

    def sync():
        side.synchronize()
        torch.cuda.synchronize()                                  # torch's own fills and uploads run on its stream

    rekey_in_use(hx, own, dev, orc, sync)
    own.use_own_stream()
    own.close()


def test_refusals_leave_every_object_as_it_was(hx, ctx, dev, orc):
    n, L, K, alpha = 1024, 3, 5, 2
    env = Env(hx, ctx, dev, orc, n, L, K, orc.primes(K, 51, n))
    other = Env(hx, ctx, dev, orc, n, L, K, orc.primes(K, 51, n))      # the same parameters, another plan
    keyed, bare, foreign = env.obj(alpha), env.obj(1), other.obj(alpha)
    keyed.gen_relin_keys(env.sec, seed=SEED, stream=3)
    before = env.exported(keyed)
    lib = hx.lib()
    seed_ok, _ = hx.seed_words(SEED)
    S, F = env.sec.data_ptr(), env.poly.data_ptr()
    vp, u64, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int

    def call(objs, kinds, elts=None, froms=None, secret=S, seed=seed_ok, first=0, n_keys=None):
        handles = (vp * len(objs))(*[None if o is None else o.h.value for o in objs])
        return lib.hexl_hks_keygen(handles, len(objs) if n_keys is None else n_keys, (ci * len(kinds))(*kinds),
                                   None if elts is None else (u64 * len(elts))(*elts), None if froms is None else (vp * len(froms))(*froms),
                                   secret, seed, 0, first)

    pair = [keyed, bare]
    refused = {
        "objects on two plans": lambda: call([keyed, bare, foreign], [SQUARE] * 3),
        "a repeated object": lambda: call([keyed, bare, keyed], [SQUARE] * 3),
        "an even Galois element": lambda: call(pair, [SQUARE, GALOIS], elts=[5, 4]),
        "a Galois element >= 2n": lambda: call(pair, [GALOIS, SQUARE], elts=[2 * n + 1, 5]),
        "GALOIS without elements": lambda: call(pair, [SQUARE, GALOIS]),
        "POLY with a null entry": lambda: call(pair, [POLY, POLY], froms=[F, None]),
        "POLY without polynomials": lambda: call(pair, [SQUARE, POLY]),
        "an unknown kind": lambda: call(pair, [SQUARE, 3]),
        "a negative kind": lambda: call(pair, [-1, SQUARE]),
        "a null object": lambda: call([keyed, None], [SQUARE, SQUARE]),
        "no secret": lambda: call(pair, [SQUARE, SQUARE], secret=None),
        "no seed": lambda: call(pair, [SQUARE, SQUARE], seed=None),
        "no key": lambda: call(pair, [SQUARE, SQUARE], n_keys=0),
        "first + sum dnum > 2^40": lambda: call(pair, [SQUARE, SQUARE], first=(1 << 40) - keyed.dnum - bare.dnum + 1),
        "first = 2^64 - 1": lambda: call(pair, [SQUARE, SQUARE], first=(1 << 64) - 1),
    }
    out = minus_one(dev, bare.dnum * 2 * K * n)
    for what, f in refused.items():
        assert f() == HEXL_E_BADARG, what
        assert lib.hexl_hks_export_keys(bare.h, out.data_ptr()) == HEXL_E_NOKEYS, f"{what}: the unkeyed object answers as if it had a key"
        assert lib.hexl_hks_export_keys(foreign.h, out.data_ptr()) == HEXL_E_NOKEYS, what
    many = [env.obj(3) for _ in range(65)]
    assert call(many, [SQUARE] * 65) == HEXL_E_BADARG, "65 keys"
    assert lib.hexl_hks_export_keys(many[0].h, out.data_ptr()) == HEXL_E_NOKEYS
    assert lib.hexl_hks_export_keys(keyed.h, None) == HEXL_E_BADARG and lib.hexl_hks_export_keys(None, out.data_ptr()) == HEXL_E_BADARG
    ctx.sync()
    assert bool((out == -1).all()), "a refusal wrote"
    same_words(env.exported(keyed), before, env, "the keyed object after the refusals")
    # accepted: first + sum dnum == 2^40, and 64 keys in one call
    assert call(pair, [SQUARE, SQUARE], first=(1 << 40) - keyed.dnum - bare.dnum) == 0
    assert call(many[:64], [SQUARE] * 64) == 0
    ctx.sync()
    same_words(env.exported(many[63]), env.wrapper_words(3, SQUARE, 1, 0, 63), env, "the last of 64 keys")
    other.close()
    env.close()


def centred_noise(lm, qs, got, want, l, n):
    """the centred CRT lift over l limbs of INTT(got - want), its largest magnitude"""
    Q = 1
    for q in qs[:l]:
        Q *= q
    acc = np.zeros(n, dtype=object)
    for i in range(l):
        q = qs[i]
        c = lm.intt(np.array((got[i].astype(object) - want[i]) % q, dtype=np.uint64), i).astype(object)
        acc = acc + c * ((Q // q) * pow(Q // q, -1, q))
    return max(min(int(v), Q - int(v)) for v in acc % Q)


def test_end_to_end_relinearize_within_the_noise_bound(hx, ctx, dev, orc):
    """hks_keygen(SQUARE); a = (0, t_a) and b = (0, t_b) with uniform t: hexl_ct_tensor_sum gives (0, 0, t_a t_b), hexl_hks_relinearize
    switches it, and hexl_rlwe_decrypt under s equals t_a t_b s^2 up to a noise within B = 21 n sum_d |G_d| D_d / P + (n_p + 1/2)(n + 1)
    (tests/hks_model.py noise_bound, the bound of test_gpu_hks.py's end-to-end test) at l = L and l = L - 1"""
    n, L, K, alpha = 1024, 4, 6, 2
    env = Env(hx, ctx, dev, orc, n, L, K, orc.primes(K, 45, n))
    plan, qs = env.plan, env.qs
    h = env.obj(alpha)
    hx.hks_keygen([h], env.sec, [SQUARE], seed=SEED, stream=2)
    model = Hks(orc, n, L, K, alpha, qs)
    s2 = env.s_from(SQUARE, 1)
    for l in (L, L - 1):
        ta, tb = [np.stack([orc.splitmix(n, 31 + 7 * l + 100 * w + i, qs[i]) for i in range(l)]) for w in range(2)]
        zero = np.zeros((1, l, n), dtype=np.uint64)
        d_a, d_b = up(hx, dev, np.concatenate([zero, ta[None]])), up(hx, dev, np.concatenate([zero, tb[None]]))
        ct3, out = minus_one(dev, 3 * l * n), minus_one(dev, 2 * l * n)
        plan.ct_tensor_sum(ct3, [d_a], [d_b], 1, l)
        h.relinearize(out, ct3, 1, l)
        dec, exp = minus_one(dev, l * n), minus_one(dev, l * n)
        plan.rlwe_decrypt(dec, out, env.sec, 1, 2, l)
        prod = np.stack([np.array(ta[i].astype(object) * tb[i].astype(object) % qs[i], dtype=np.uint64) for i in range(l)])
        plan.multiply_plain(exp, up(hx, dev, prod), s2, 1, 1, l, 1)
        ctx.sync()
        assert np.array_equal(hx.to_u64(ct3).reshape(3, l, n)[2], prod), "the tensor's third component"
        worst = centred_noise(model.lm, qs, hx.to_u64(dec).reshape(l, n), hx.to_u64(exp).reshape(l, n).astype(object), l, n)
        B = model.noise_bound(l)
        print(f"[hks keygen] relinearize level {l}: |noise| = {worst}, bound {B:.4g}")
        assert worst <= B, f"level {l}: {worst} > {B}"
    env.close()


def test_end_to_end_linear_transform_within_the_noise_bound(hx, ctx, dev, orc):
    """two Galois keys (g = 5, 2n - 1) from ONE hks_keygen call; a uniform ciphertext, dense plaintexts with |coefficient| <= 8 and an
    identity term: hexl_rlwe_decrypt of hexl_hks_linear_transform's output equals sum_r pt_r sigma_r(c0 + c1 s) + pt_id (c0 + c1 s) up to
    a noise within B_lt (hks_hoisted_model.lt_noise_bound, the bound of test_gpu_hks_hoisted.py's end-to-end test) at l = L and L - 1"""
    n, L, K, alpha = 1024, 4, 6, 2
    gs = [5, 2 * n - 1]
    env = Env(hx, ctx, dev, orc, n, L, K, orc.primes(K, 45, n))
    plan, qs = env.plan, env.qs
    objs = [env.obj(alpha), env.obj(alpha)]
    hx.hks_keygen(objs, env.sec, [GALOIS, GALOIS], galois_elts=gs, seed=SEED, stream=2)
    m = Hks(orc, n, L, K, alpha, qs)
    rng = np.random.default_rng(5)
    polys = [rng.integers(-8, 9, n) for _ in gs]
    pts = [hks_hoisted_model.encode_small(m, poly) for poly in polys]
    pt_id = hks_hoisted_model.encode_small(m, rng.integers(-8, 9, n))
    d_pts, d_id = [up(hx, dev, x) for x in pts], up(hx, dev, pt_id)
    for l in (L, L - 1):
        ct = np.concatenate([orc.splitmix(n, 5003 + 97 * l + 17 * k + i, qs[i]) for k in range(2) for i in range(l)])
        d_ct, out = up(hx, dev, ct), minus_one(dev, 2 * l * n)
        hx.hks_linear_transform(objs, gs, d_pts, d_id, out, d_ct, 1, l)
        dec, dec_in = minus_one(dev, l * n), minus_one(dev, l * n)
        plan.rlwe_decrypt(dec, out, env.sec, 1, 2, l)
        plan.rlwe_decrypt(dec_in, d_ct, env.sec, 1, 2, l)
        ctx.sync()
        got, msg = hx.to_u64(dec).reshape(l, n), hx.to_u64(dec_in).reshape(l, n)
        want = []
        for i in range(l):
            w = pt_id[i].astype(object) * msg[i].astype(object)
            for g, pt in zip(gs, pts):
                w = w + pt[i].astype(object) * apply_galois(msg[i], n, g).astype(object)
            want.append(w)
        worst = centred_noise(m.lm, qs, got, want, l, n)
        B = hks_hoisted_model.lt_noise_bound(m, l, [int(np.abs(poly).sum()) for poly in polys])
        print(f"[hks keygen] linear transform level {l}: |noise| = {worst}, bound {B:.4g}")
        assert worst <= B, f"level {l}: {worst} > {B}"
    env.close()
