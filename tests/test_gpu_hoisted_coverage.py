"""GPU: the hoisted rotation family -- hexl_rotate_hoisted, hexl_linear_transform, hexl_linear_transform_bsgs -- at every ring size, FP64
tier and digit count the entry points accept, word for word against the exact models (hoist_model.rotate_hoisted,
lt_model.linear_transform, bsgs_model.linear_transform_bsgs; pinned to the oracle in test_hoist_model.py, test_lt_model.py and
test_bsgs_model.py), every instance, compared on the device. There is no tolerance anywhere. Every output buffer starts as -1.

A "triple" is the three entry points on the same plans and the same two distinct ciphertexts, the model's mod-up computed once per
ciphertext and shared by all three:
    hexl_rotate_hoisted         g = 5^3 mod 2n and 2n - 1
    hexl_linear_transform       the same two, one plaintext each, and an identity term
    hexl_linear_transform_bsgs  2 x 2: baby steps 3 and 2n - 1, giant steps G = 1 and G = 3 (other keys than the baby 3)
The `uniform` family draws every word uniformly below its modulus; `extreme` takes ks_util.extreme_words (q - 1, the words beside q / 2,
0, 1) for the ciphertext, the keys and the plaintexts alike. What the sibling files leave unrun and this one runs:
    every geometry          n = 2048 (KL = 1) and 8192 (KL = 3) in both families; `extreme` at 4096, 16384, 32768
    every tier at 16384     ks_util.EXTREME_TIERS at L = 3: periods 3, 6 and 12, strict below 2^52 and just above 2^51 + 2^44, two mixed
                            chains; the fused mod-up (k_ksf_up<., CT>) on periods 6 and 12 and on the strict tier
    per-limb lookup         HEXL_KS_PER_LIMB=2 in a child process: the LAZY = -1 kernels on the two mixed chains
    digit counts            L = 1, L = 8 (the last of the 8-digit multiply-accumulate), L = 15 (the largest plan)
    K > L + 1               the special prime is plan modulus K - 1, not L; g = 1 pinned to the oracle's keyswitch
    long sums               16 rotations and an 8 x 2 grid of worst-case words, at 51 bits and just below 2^52
Helpers of the three sibling files are reused by import."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import test_gpu_linear_transform as lt
import test_gpu_linear_transform_bsgs as bs
import test_gpu_rotate_hoisted as rh
from bsgs_model import linear_transform_bsgs
from ckks_model import rotate
from hoist_model import limbs_of, mod_up, rotate_hoisted
from ks_util import EXTREME_TIERS, extreme_ciphertext, tier_moduli
from lt_model import linear_transform, uniform_plaintext
from test_gpu_linear_transform import extreme_plaintext
from test_gpu_rotate_hoisted import cases_for, made, plans_for, torch_, uniform_ct  # noqa: F401  (made: a fixture)

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# what plan.tiers() reports for K = 4 limbs at n = 16384 in each of ks_util.EXTREME_TIERS: the schedule the tier's name says
TIER_PERIODS = {
    "skip_period3_51bit": ([3, 3, 3, 3], False),
    "period3_tier_top_2^51_plus_2^44": ([3, 3, 3, 3], False),
    "strict_just_above_2^51_plus_2^44": ([0, 0, 0, 0], False),
    "skip_period6_just_below_2^50": ([6, 6, 6, 6], False),
    "skip_period12_just_below_2^49": ([12, 12, 12, 12], False),
    "strict_just_below_2^52": ([0, 0, 0, 0], False),
    "mixed_seal_chain_strict_and_period12": ([0, 12, 12, 12], True),
    "mixed_all_four_tiers": ([0, 3, 6, 12], True),
}
assert sorted(TIER_PERIODS) == sorted(EXTREME_TIERS)


def plans_of(hx, ctx, cases, made_):
    """one plan with keys per case. K = L + 1: plans_for; K > L + 1: rns_modulus_size = L + 1 (case.rns), as test_gpu_keyswitch.py's
    test_vs_oracle builds its (4096, 5, 7) plan -- plans_for passes K there"""
    if cases[0].K == cases[0].L + 1:
        return plans_for(hx, ctx, cases, made_)
    plans = []
    for case in cases:
        plan = hx.KeySwitchPlan(ctx, case.n, case.L, case.K, case.rns, 2, case.moduli, case.modswitch)
        made_.append(plan)
        plan.set_keys(case.keys)
        plans.append(plan)
    return plans


class Inputs:
    """two distinct ciphertexts of one family, the plaintexts drawn from the same family, and the model's mod-up of each ciphertext --
    computed here once and shared by every entry point that meets these ciphertexts"""

    def __init__(self, orc, case, family, distinct=2):
        assert family in ("uniform", "extreme"), family
        self.orc, self.case, self.ext = orc, case, family == "extreme"
        self.cts = [extreme_ciphertext(case, b, 2) if self.ext else uniform_ct(orc, case, b) for b in range(distinct)]
        self.lm = limbs_of(orc, case)
        self.ups = [mod_up(self.lm, case, ct) for ct in self.cts]

    def pt(self, s):
        """[L + 1][n], row L below the special prime moduli[K - 1]"""
        return extreme_plaintext(self.case, 1 + s) if self.ext else uniform_plaintext(self.orc, self.case, s)

    def pt_id(self, s):
        L = self.case.L
        return extreme_plaintext(self.case, 5 + s, rows=L) if self.ext else uniform_plaintext(self.orc, self.case, 9 + s, rows=L)

    def want_rotations(self, cases, gs):
        return [[rotate_hoisted(self.orc, c, ct, g, self.lm, u) for ct, u in zip(self.cts, self.ups)] for c, g in zip(cases, gs)]

    def want_lt(self, cases, gs, pts, pt_id):
        return [linear_transform(self.orc, cases, gs, pts, pt_id, ct, self.lm, u) for ct, u in zip(self.cts, self.ups)]

    def want_bsgs(self, bcases, bgs, gcases, ggs, pts, pt_ids):
        return [linear_transform_bsgs(self.orc, bcases, bgs, gcases, ggs, pts, pt_ids, ct, self.lm, u) for ct, u in zip(self.cts, self.ups)]


def check_rotations(hx, ctx, dev, inp, cases, plans, gs, nb, label=""):
    d_ct, outs = rh.buffers(hx, dev, inp.cts, nb, len(gs))
    hx.rotate_hoisted(plans, gs, outs, d_ct, nb)
    ctx.sync()
    rh.assert_outputs(hx, inp.want_rotations(cases, gs), outs, nb, cases[0], label + "rotate_hoisted: ")
    return d_ct, outs


def check_lt(hx, ctx, dev, inp, cases, plans, gs, pts, pt_id, nb, label=""):
    want = inp.want_lt(cases, gs, pts, pt_id)
    return lt.run_and_check(hx, ctx, dev, inp.orc, cases, plans, gs, pts, pt_id, inp.cts, nb, want=want, label=label + "linear_transform: ")


def check_bsgs(hx, ctx, dev, inp, bcases, bplans, bgs, gcases, gplans, ggs, pts, pt_ids, nb, label="", composition=False):
    want = inp.want_bsgs(bcases, bgs, gcases, ggs, pts, pt_ids)
    ref = inp.case
    d_ct, out, d_pts, d_ids = bs.run_and_check(hx, ctx, dev, want, ref, bplans, bgs, gplans, ggs, pts, pt_ids, inp.cts, nb,
                                               label=label + "linear_transform_bsgs: ")
    if composition:
        comp = bs.device_composition(hx, ctx, ref, bplans, bgs, gplans, ggs, d_pts, d_ids, d_ct, nb)
        assert np.array_equal(hx.to_u64(out).reshape(nb, -1), comp), label + "not the device composition's words"


def triple(hx, ctx, dev, orc, cases, plans, family, nb=3, label="", composition=False, inp=None):
    """the three entry points on cases / plans [0 ... 2] (2: the giant step's keys), then the range flags"""
    ref = cases[0]
    n = ref.n
    inp = inp or Inputs(orc, ref, family)
    gs = [pow(5, 3, 2 * n), 2 * n - 1]
    check_rotations(hx, ctx, dev, inp, cases[:2], plans[:2], gs, nb, label)
    check_lt(hx, ctx, dev, inp, cases[:2], plans[:2], gs, [inp.pt(0), inp.pt(1)], inp.pt_id(0), nb, label)
    if not inp.ext:                                                    # (worst-case keys are the same words in every key set)
        assert not np.array_equal(cases[0].keys[0], cases[2].keys[0]), "the baby 3 and the giant 3 take different keys"
    check_bsgs(hx, ctx, dev, inp, cases[:2], plans[:2], [3, 2 * n - 1], [None, cases[2]], [None, plans[2]], [1, 3],
               [[inp.pt(2), inp.pt(3)], [inp.pt(4), inp.pt(5)]], None, nb, label, composition)
    assert all(p.range_check() for p in plans), label + "in-range words must not raise a range flag"
    return inp


def triple_case(hx, ctx, dev, orc, made_, n, L, K, family, moduli=None, nb=3, composition=False):
    cases = cases_for(orc, n, L, K, 3, moduli=moduli, extreme_keys=family == "extreme")
    plans = plans_of(hx, ctx, cases, made_)
    return cases, plans, triple(hx, ctx, dev, orc, cases, plans, family, nb, composition=composition)


# ---- 1. every geometry: hx_with_f64_geom's six (logn, LOGE) pairs; KL = 1 (n = 2048) and KL = 3 (n = 8192) occur nowhere else ----
@pytest.mark.parametrize("family", ["uniform", "extreme"])
@pytest.mark.parametrize("n", [2048, 8192])
def test_the_two_geometries_no_sibling_runs(hx, ctx, dev, orc, made, n, family):
    """posB, the gather of k_ksf_mac_galois, k_lt_bsgs_sum, the piece decode of k_galois_c0_pt / k_galois_add and the in-place reads of
    k_ksf_intt<., CT> all depend on the geometry. n = 2048: also against the composition on the device, which involves no model"""
    triple_case(hx, ctx, dev, orc, made, n, 2, 3, family, composition=n == 2048)


@pytest.mark.parametrize("n", [4096, 16384, 32768])
def test_worst_case_words_on_the_other_rings(hx, ctx, dev, orc, made, n):
    """the sibling files run these rings on uniform words only"""
    triple_case(hx, ctx, dev, orc, made, n, 2, 3, "extreme")


# ---- 2. every tier at n = 16384, the only ring with the period-6 and period-12 schedules ----
def tier_case(hx, ctx, orc, made_, tier, family):
    n, L, K = 16384, 3, 4
    cases = cases_for(orc, n, L, K, 3, moduli=tier_moduli(orc, tier, n, K), extreme_keys=family == "extreme")
    plans = plans_of(hx, ctx, cases, made_)
    return cases, plans


@pytest.mark.parametrize("tier", EXTREME_TIERS)
def test_every_tier_worst_case_words(hx, ctx, dev, orc, made, tier):
    """batch 3: k_ksf_intt<., CT> + k_ksf_ntt_up. Just below 2^52 is the tightest case of lt_mac_acc (|prev + product| <= 1.2 p + 2
    against 2^53) and of the 52-bit word conversions"""
    cases, plans = tier_case(hx, ctx, orc, made, tier, "extreme")
    assert plans[0].tiers() == TIER_PERIODS[tier], f"{tier}: the plan does not select the schedule the tier is named for"
    triple(hx, ctx, dev, orc, cases, plans, "extreme", label=tier + ": ")


@pytest.mark.parametrize("tier", ["skip_period6_just_below_2^50", "skip_period12_just_below_2^49", "strict_just_below_2^52"])
def test_fused_mod_up_in_the_tiers_the_siblings_leave_out(hx, ctx, dev, orc, made, tier):
    """the smallest batch with nb * L >= 2 * CUs, inside one scratch chunk: k_ksf_up<14, 4, 6 / 12 / 0, CT> for the ciphertext's mod-up
    and for the giant step's"""
    cases, plans = tier_case(hx, ctx, orc, made, tier, "uniform")
    assert plans[0].tiers() == TIER_PERIODS[tier]
    L = cases[0].L
    cus = int(ctx.describe().split(" CUs")[0].split()[-1])
    assert cus == torch_().cuda.get_device_properties(0).multi_processor_count
    nb = -(-2 * cus // L)
    chunk = plans[0].scratch_bytes(1 << 24) // plans[0].scratch_bytes(1)
    assert nb * L >= 2 * cus and (nb - 1) * L < 2 * cus and nb <= chunk, "one scratch chunk, on the fused route"
    assert hx.lt_bsgs_scratch_bytes(plans[0], 2, nb) == nb * hx.lt_bsgs_scratch_bytes(plans[0], 2, 1), "one chunk of the baby store too"
    triple(hx, ctx, dev, orc, cases, plans, "uniform", nb=nb, label=tier + ": ")


# ---- 3. the per-limb lookup kernels (LAZY = -1): HEXL_KS_PER_LIMB is read once per process ----
MIXED_CHAINS = ["mixed_all_four_tiers", "mixed_seal_chain_strict_and_period12"]          # tier_ladder and seal_chain


@pytest.mark.parametrize("tier", MIXED_CHAINS)
def test_mixed_chains_on_the_plan_wide_tier(hx, ctx, dev, orc, made, tier):
    """the default knob: a plan of mixed tiers runs the (b, d)-major kernels of its most careful limb's tier. Uniform words here; the
    worst-case family on these two chains is test_every_tier_worst_case_words"""
    cases, plans = tier_case(hx, ctx, orc, made, tier, "uniform")
    assert plans[0].tiers() == TIER_PERIODS[tier]
    triple(hx, ctx, dev, orc, cases, plans, "uniform", label=tier + ": ")


def test_mixed_chains_on_the_per_limb_lookup_kernels():
    """HEXL_KS_PER_LIMB=2 in a child process: ksf_lazy returns -1 for a plan of mixed tiers, so the hoisted callers run
    k_ksf_intt<14, 4, -1, CT>, k_ksf_ntt_up, k_ksf_intt_sp and k_ksf_moddown with the schedule looked up per transform. The two chains of
    test_mixed_chains_on_the_plan_wide_tier in both families, against the same model words as under the default knob"""
    code = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import torch, hexl_fpga_amd as hx, orc
from test_gpu_hoisted_coverage import MIXED_CHAINS, TIER_PERIODS, tier_case, triple
dev = torch.device("cuda:0")
ctx = hx.Context(0)
made = []
for tier in MIXED_CHAINS:
    for family in ("uniform", "extreme"):
        cases, plans = tier_case(hx, ctx, orc, made, tier, family)
        assert plans[0].tiers() == TIER_PERIODS[tier] and plans[0].tiers()[1], "mixed tiers expected"
        triple(hx, ctx, dev, orc, cases, plans, family, label="%%s, %%s: " %% (tier, family))
        print("OK", tier, family, flush=True)
torch.cuda.synchronize()
for o in reversed(made):
    o.close()
print("PER LIMB OK")
''' % (str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, HEXL_KS_PER_LIMB="2"))
    print(out.stdout[-1000:], out.stderr[-1500:])
    assert out.returncode == 0 and "PER LIMB OK" in out.stdout


# ---- 4. digit-count edges at n = 1024 ----
@pytest.mark.parametrize("family", ["uniform", "extreme"])
@pytest.mark.parametrize("L", [1, 8])
def test_one_digit_and_the_last_eight_digit_plan(hx, ctx, dev, orc, made, L, family):
    """L = 1: every L * L and (L + 1) * L stride degenerates. L = 8: the last L of ksf_with_maxl's 8-digit instantiation.
    L = 1 also with g = 1 in the rotation list: hexl_rotate's words and the oracle's keyswitch"""
    n, K, nb = 1024, L + 1, 3
    cases, plans, inp = triple_case(hx, ctx, dev, orc, made, n, L, K, family, nb=nb)
    if L == 1:
        gs = [1, pow(5, 3, 2 * n), 2 * n - 1]
        d_ct, outs = check_rotations(hx, ctx, dev, inp, cases, plans, gs, nb, "with g = 1: ")
        d_rot = torch_().full_like(d_ct, -1)
        plans[0].rotate(d_rot, d_ct, nb, 1)
        ctx.sync()
        assert torch_().equal(d_rot, outs[0]), "g = 1 must give hexl_rotate's words"
        assert np.array_equal(hx.to_u64(outs[0]).reshape(nb, -1)[1], rotate(orc, cases[0], inp.cts[1], 1))
        assert all(p.range_check() for p in plans)


def test_the_largest_plan(hx, ctx, dev, orc, made):
    """L = 15, K = 16: the triple on uniform words, then one linear transform with three rotations of worst-case words (other plans: the
    keys are worst-case too)"""
    n, L, K, nb = 1024, 15, 16, 3
    triple_case(hx, ctx, dev, orc, made, n, L, K, "uniform", nb=nb)
    cases = cases_for(orc, n, L, K, 3, extreme_keys=True)
    plans = plans_of(hx, ctx, cases, made)
    inp = Inputs(orc, cases[0], "extreme")
    check_lt(hx, ctx, dev, inp, cases, plans, [3, pow(5, 3, 2 * n), 2 * n - 1], [inp.pt(r) for r in range(3)], inp.pt_id(0), nb, "extreme: ")
    assert all(p.range_check() for p in plans)


# ---- 5. K > L + 1: the special prime is plan modulus K - 1, the keys are [K] rows on the host and [L + 1] on the device ----
@pytest.mark.parametrize("family", ["uniform", "extreme"])
@pytest.mark.parametrize("n,L,K", [(1024, 2, 4), (4096, 5, 7)])
def test_more_key_moduli_than_digits_plus_one(hx, ctx, dev, orc, made, n, L, K, family):
    """an L written where K - 1 belongs -- a modulus, a table, a key row, row L of a plaintext -- gives other words here, and only here.
    g = 1 anchors the model outside itself: hexl_rotate_hoisted's words are the oracle's keyswitch"""
    nb = 3
    cases, plans, inp = triple_case(hx, ctx, dev, orc, made, n, L, K, family, nb=nb)
    assert int(cases[0].moduli[L]) != int(cases[0].moduli[K - 1])
    d_ct, outs = rh.buffers(hx, dev, inp.cts, nb, 1)
    hx.rotate_hoisted(plans[:1], [1], outs, d_ct, nb)
    ctx.sync()
    got = hx.to_u64(outs[0]).reshape(nb, -1)
    for b in range(nb):
        assert np.array_equal(got[b], rotate(orc, cases[0], inp.cts[b % 2], 1)), f"g = 1, instance {b}: not the oracle's keyswitch"
    assert all(p.range_check() for p in plans)


# ---- 6. long accumulation chains of worst-case words ----
@pytest.mark.parametrize("n,tier", [(1024, "skip_period3_51bit"), (16384, "strict_just_below_2^52")])
def test_long_sums_of_worst_case_words(hx, ctx, dev, orc, made, n, tier):
    """16 rotations with the identity term through lt_mac_acc in k_ksf_mac_galois and k_galois_c0_pt, then an 8 x 2 grid with every diagonal
    present: k_lt_bsgs_sum walks 8 terms per row. Every ciphertext, key and plaintext word is q - 1, beside q / 2, 0 or 1"""
    L, K, nb = 2, 3, 3
    R = 16
    cases = cases_for(orc, n, L, K, R, moduli=tier_moduli(orc, tier, n, K), extreme_keys=True)
    plans = plans_of(hx, ctx, cases, made)
    if n == 16384:
        assert plans[0].tiers() == ([0, 0, 0], False), "the true strict tier"
    inp = Inputs(orc, cases[0], "extreme")
    gs = [pow(5, k, 2 * n) for k in range(1, R)] + [2 * n - 1]
    assert len(set(gs)) == R
    check_lt(hx, ctx, dev, inp, cases, plans, gs, [inp.pt(r) for r in range(R)], inp.pt_id(0), nb, "16 rotations: ")
    bgs, ggs = gs[:7] + [2 * n - 1], [1, 3]
    pts = [[inp.pt(8 * j + i) for i in range(8)] for j in range(2)]
    check_bsgs(hx, ctx, dev, inp, cases[:8], plans[:8], bgs, [None, cases[8]], [None, plans[8]], ggs, pts, None, nb, "8 x 2 grid: ")
    assert all(p.range_check() for p in plans)
