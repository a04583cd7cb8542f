/*
 * hexl_mi355x.h -- C-ABI of the MI355X (gfx950) launcher library libhexl_mi355x.so.
 *
 * This is the drop-in boundary for the hexl-fpga hot path. In the reference the same seam is
 * the dlopen'ed "bitstream" launcher table (host/inc/dl_kernel_interfaces.hpp:45-136,
 * device/fwd_ntt.cpp:619-646, device/inv_ntt.cpp:577-607, device/dyadic_multiply.cpp:349-405,
 * device/keyswitch.cpp:15-65) whose signatures carry sycl::queue& / sycl::buffer&; here it is
 * plain C: opaque handles, raw pointers and sizes, int status (0 = ok, else hipError_t or
 * a negative HEXL_E_* code). No torch / C++ types cross it.
 *
 * Pointers named d_* are DEVICE pointers (HBM), h_* are HOST pointers.
 * All launchers are asynchronous on the context's stream; hexl_ctx_sync() waits.
 *
 * The C++ API of the reference (host/inc/hexl-fpga.h:15-161, namespace intel::hexl) is built on
 * top of these entry points in libhexl-fpga.so (see include/hexl-fpga.h).
 */
#ifndef HEXL_MI355X_H
#define HEXL_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HEXL_E_BADARG   (-1)   /* unsupported n / null pointer / size limit */
#define HEXL_E_NOKEYS   (-2)   /* hexl_keyswitch before hexl_ks_set_keys */
#define HEXL_E_NODEVICE (-3)   /* no gfx950 device visible */
#define HEXL_E_RANGE    (-4)   /* HEXL_KS_VALIDATE=1: a t_target / result word is not below its modulus; the call was REFUSED, nothing computed */
#define HEXL_W_RANGE    1      /* status, not an error: the call ran, but the FP64 kernels saw a t_target / result word that is not below its
                                  modulus (hexl_ks_range_check, hexl_keyswitch_host); the output words of such an object are unspecified */

typedef struct hexl_ctx hexl_ctx;         /* one per GPU: stream + scratch */
typedef struct hexl_ks_plan hexl_ks_plan; /* keyswitch parameter set: tables + keys on device */

/* number of gfx950 devices visible to the process (0 if none); what NUM_DEV is clamped to
 * (DevicePool, host/src/fpga.cpp:1646-1673) */
int hexl_device_count(void);

/* replaces acquire_/release_FPGA_resources' device half (host/src/fpga.cpp:1646-1685):
 * binds `device`, creates the stream. */
int hexl_ctx_create(int device, hexl_ctx** out);
int hexl_ctx_destroy(hexl_ctx* ctx);
/* run on a caller-owned hipStream_t (e.g. torch's current stream; NULL = the legacy default stream).
 * Stream switches are ordered: after hexl_ctx_set_stream or hexl_ctx_use_own_stream, work submitted through the context and its plans on
 * the new stream runs behind everything the context has submitted on the previous stream (the context and its plans keep one set of
 * scratch buffers, which the next launch rewrites). The call itself does not block the host, and does nothing when the stream does
 * not change. The previous stream must still exist at the switch: switch away from a stream before destroying it. The caller's own
 * buffers are the caller's to order, as between any two streams. NULL ctx: HEXL_E_BADARG. */
int hexl_ctx_set_stream(hexl_ctx* ctx, void* hip_stream);
/* go back to the context's own non-blocking stream (the state after hexl_ctx_create); ordered like hexl_ctx_set_stream */
int hexl_ctx_use_own_stream(hexl_ctx* ctx);
int hexl_ctx_sync(hexl_ctx* ctx);
/* library/device report for logs: writes a NUL-terminated string */
int hexl_ctx_describe(hexl_ctx* ctx, char* buf, size_t buflen);

/* K1 -- batched negacyclic forward NTT, in place, bit-exact with fwd_ntt_kernel
 * (device/fwd_ntt.cpp:82-497; launchers fwd_ntt/ntt_input/ntt_output :619-646).
 * d_x[batch][n]; one modulus and one table pair (bit-reversed order, n words each) per batch.
 * n in {1024, 2048, 4096, 8192, 16384, 32768} (reference: 16384 only, host/src/ntt.cpp:24). */
int hexl_ntt_fwd(hexl_ctx* ctx, uint64_t* d_x, size_t batch, const uint64_t* d_roots,
                 const uint64_t* d_precon, uint64_t q, uint64_t n);

/* K2 -- batched inverse NTT, in place, bit-exact with inv_ntt_kernel
 * (device/inv_ntt.cpp:83-441; launchers :577-607). Inverse tables in the HEXL layout
 * (stage-major, first used entry at index 1); inv_n, inv_n_w caller scalars
 * (host/inc/hexl-fpga.h:150-154). */
int hexl_ntt_inv(hexl_ctx* ctx, uint64_t* d_x, size_t batch, const uint64_t* d_inv_roots,
                 const uint64_t* d_inv_precon, uint64_t q, uint64_t inv_n, uint64_t inv_n_w,
                 uint64_t n);

/* K3 -- batched dyadic ciphertext multiply (device/dyadic_multiply.cpp:61-342, launchers
 * :349-405). d_a/d_b[batch][2][n_moduli][n], d_out[batch][3][n_moduli][n],
 * d_moduli[batch][n_moduli]. Exact for any 64-bit operands, moduli in [2, 2^62). */
int hexl_dyadic_multiply(hexl_ctx* ctx, uint64_t* d_out, const uint64_t* d_a,
                         const uint64_t* d_b, size_t batch, uint64_t n,
                         const uint64_t* d_moduli, uint64_t n_moduli);

/* K4 -- keyswitch. The plan replaces the reference's per-parameter-set device state:
 * build_modulus_meta / build_invn_meta / KeySwitch_load_twiddles (host/src/fpga.cpp:1049-1123)
 * and KeySwitch_load_keys (:1167-1248).
 *   n in {1024..16384}; 1 <= L < K <= 16; key_component_count == 2; moduli < 2^60
 *   (reference: K <= 7, moduli <= 2^52, host/src/keyswitch.cpp:23-34).
 *   h_moduli[K], h_modswitch[K]; h_twiddles = K blocks of 4n words
 *   [inv_roots | precon_inv | roots | precon_roots] in the hexl-fpga layout
 *   (host/src/twiddle-factors.cpp:16-62) or NULL to derive them from
 *   MinimalPrimitiveRoot(2n, q_i) as fpga.cpp:1097-1109 does. */
int hexl_ks_plan_create(hexl_ctx* ctx, uint64_t n, uint64_t decomp_modulus_size,
                        uint64_t key_modulus_size, uint64_t rns_modulus_size,
                        uint64_t key_component_count, const uint64_t* h_moduli,
                        const uint64_t* h_modswitch, const uint64_t* h_twiddles,
                        hexl_ks_plan** out);
int hexl_ks_plan_destroy(hexl_ks_plan* plan);
/* h_keys[d] -> key words k_switch_keys[d][(k*K + i)*n + j] (fpga.cpp:1186-1190), d < L */
int hexl_ks_set_keys(hexl_ks_plan* plan, const uint64_t* const* h_keys);
/* d_t_target[batch][L][n]; d_result[batch][2][L][n] is read-modify-write: the keyswitch
 * output is added into it mod q_i (fpga.cpp:441-475). Precondition, as for intel::hexl::KeySwitch:
 * every t_target / result word is below its modulus (the FP64 kernels used for moduli < 2^52 compute
 * the exact residues of in-range data; the integer kernels used for larger moduli replay the lazy
 * arithmetic on raw words instead -- out-of-range inputs are outside the contract on both).
 * With HEXL_KS_VALIDATE=1 in the environment every call first checks that precondition on the device
 * (one extra pass over the inputs and a stream synchronisation) and returns HEXL_E_RANGE without
 * touching `result` if it does not hold. Steps load -> INTT -> mod-up -> NTT ->
 * key MAC -> INTT(special) -> round -> NTT -> mod-switch -> store of
 * device/keyswitch/ (SURVEY 2.1-K4). */
int hexl_keyswitch(hexl_ks_plan* plan, uint64_t* d_result, const uint64_t* d_t_target,
                   size_t batch);
/* The FP64 kernels (moduli < 2^52) check the precondition above where they convert the words anyway -- one compare per
 * word, no extra pass -- and OR the outcome into a flag of the plan. This call waits for the plan's stream and returns
 * HEXL_W_RANGE (> 0) if any hexl_keyswitch launched on the plan since the flag was last cleared saw a t_target / result word
 * >= its modulus (the output words of that instance are then unspecified), 0 otherwise; it clears the flag. The integer
 * kernels (moduli >= 2^52) do not flag: they replay the reference's lazy arithmetic on whatever words they get.
 * hexl_keyswitch_host() reports for ITS OWN objects only: it clears the flag when it starts (call hexl_ks_range_check first
 * if earlier device-pointer launches on the plan matter) and returns HEXL_W_RANGE when one or more objects of the call had
 * an out-of-range word -- it cannot say which. HEXL_E_RANGE (< 0) is different: the HEXL_KS_VALIDATE=1 refusal, nothing ran. */
int hexl_ks_range_check(hexl_ks_plan* plan);
/* Beyond the reference's envelope (the use-case of its combined image,
 * device/dyadic_multiply_keyswitch.cpp:4-5): ciphertext multiply + relinearize in one pass.
 *   d_a, d_b [batch][2][L][n] (the DyadicMultiply operand layout with n_moduli = L, words < q_i);
 *   d_out    [batch][2][L][n] is WRITTEN with (a0 b0, a0 b1 + a1 b0) + KeySwitch(a1 b1), i.e. what
 *   DyadicMultiply followed by KeySwitch(result = components 0..1, t_target = component 2) leaves -- but the
 *   three-component product never exists in memory. n = 1024 ... 32768 and moduli < 2^52 only (else HEXL_E_BADARG).
 *   d_out must not overlap d_a or d_b (component 0 is stored before component 1's operands are read): HEXL_E_BADARG. */
int hexl_multiply_relinearize(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* d_a,
                              const uint64_t* d_b, size_t batch);
/* CKKS level operations beside hexl_multiply_relinearize: a ciphertext stays on the device through multiply + relinearize ->
 * rescale -> rotate. All three are asynchronous on the context's stream.
 *
 * Galois automorphism X -> X^galois_elt on `count` polynomials of n words each in NTT form, in the transforms' (bit-reversed) output
 * order: out[j] = in[brv(((2 brv(j) + 1) g mod 2n - 1) / 2)], brv = bit reversal over log2(n) bits. Words are moved, never interpreted:
 * any 64-bit value survives and no modulus is involved. n = 1024 ... 32768; galois_elt odd and below 2n. d_out must not overlap d_in.
 * Anything else: HEXL_E_BADARG. */
int hexl_apply_galois(hexl_ctx* ctx, uint64_t* d_out, const uint64_t* d_in, size_t count, uint64_t n, uint64_t galois_elt);
/* Rescale (SEAL's rescale_to_next): divide by the last modulus of the level and drop it, rounding to nearest.
 *   d_in  [batch][n_components][n_limbs][n]      NTT form, words < q_i, moduli = the plan's first n_limbs
 *   d_out [batch][n_components][n_limbs - 1][n]  WRITTEN with NTT_i(round(X / q_l) mod q_i), l = n_limbs - 1, X the CRT value of
 *                                                each coefficient
 * 2 <= n_limbs <= K - 1 (the last plan modulus is the special prime), 1 <= n_components <= 3; FP64 plans only (every modulus < 2^52)
 * and n = 1024 ... 32768, as hexl_multiply_relinearize; d_out must not overlap d_in. Anything else: HEXL_E_BADARG. Needs no keys.
 * The first call for a level computes that level's constants on the host and keeps them in the plan (< 8 KiB for all levels).
 * Device memory kept by the plan, grow-only: min(batch, chunk) x n_components x n doubles of scratch, chunk = 256 instances at
 * n = 16384 (the same number of coefficients at other n) -- 64 MiB for two components. */
int hexl_rescale(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* d_in, size_t batch, uint64_t n_limbs,
                 uint64_t n_components);
/* Rotate: d_ct[batch][2][L][n] -> d_out[batch][2][L][n] WRITTEN with (sigma_g(c0), 0) + KeySwitch(sigma_g(c1)), sigma_g the Galois
 * automorphism above. The plan's keys must be the switching key from s(X^g) to s (the caller's responsibility). Runs on every plan
 * hexl_keyswitch accepts, integer kernels included. HEXL_E_NOKEYS before hexl_ks_set_keys; HEXL_E_BADARG for a galois_elt that is
 * even or >= 2n, or d_out overlapping d_ct. Device memory kept by the plan, grow-only, beside the keyswitch's scratch:
 * min(batch, chunk) x L x n words (sigma_g(c1) of one slice; 224 MiB at n = 16384, L = 7), shared with hexl_relinearize and
 * hexl_multiply_sum_relinearize. */
int hexl_rotate(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* d_ct, size_t batch, uint64_t galois_elt);
/* Hoisted rotations: n_rot rotations of ONE ciphertext batch (the inner loop of the diagonal method, rotate -> multiply_plain ->
 * accumulate). The keyswitch's steps 1-2 (inverse transforms and mod-up, L + L*L of its L*L + 3L + 2 transforms) depend on c1 alone,
 * not on the key, and commute with the Galois automorphism up to a digit lift of the same size: they run once per chunk and every
 * rotation reuses their output.
 *   plans[r]        holds the switching key from s(X^g_r) to s;  galois_elts[r] = g_r
 *   d_outs          HOST array of n_rot DEVICE pointers, each [batch][2][L][n]
 *   d_ct            [batch][2][L][n], NTT form, every word below its modulus
 * For every r, d_outs[r] is WRITTEN with (sigma_g(c0), 0) + ModDown(sum_d sigma_g(u_d) . key_r[d]), where
 * u_d[slot] = NTT_slot(INTT_d(c1[d]) mod q_slot) is the keyswitch's mod-up of c1, sigma_g the word permutation of hexl_apply_galois
 * and ModDown the keyswitch's steps 4-7. Asynchronous on the context's stream (one lane: the stream contract of hexl_ctx_set_stream
 * holds as for any single launch).
 * NOT word-identical to hexl_rotate for g != 1: hexl_rotate lifts the digits of sigma_g(c1), where a negated coefficient is q_d - c
 * before it is reduced modulo q_i; this call lifts the digits of c1 and then permutes, where it is -(c mod q_i). The two differ by
 * multiples of q_d inside a digit; both are digit lifts below q_d that are congruent to sigma_g(c1) modulo q_d, so both outputs
 * decrypt to the same plaintext with key-switch noise of the same bound. For g = 1 the output is word for word that of hexl_rotate.
 * Plans: all of one context, with the same n, L, K and moduli; FP64 plans only (every modulus < 2^52), n = 1024 ... 32768; every
 * plan with keys (else HEXL_E_NOKEYS). The plans must have been created with the same twiddles (all derived, or the same h_twiddles):
 * that is the caller's responsibility, it is not checked. The same g, or the same plan, may appear more than once.
 * HEXL_E_BADARG: a null pointer (in the arguments or in either array), a plan that does not match plans[0] or runs on the integer
 * kernels, a g that is even or >= 2n, a d_outs[r] that overlaps d_ct or another d_outs[r'], a size that overflows. n_rot == 0 or
 * batch == 0 returns 0 after these checks and writes nothing.
 * Device memory: steps 1-2 run in plans[0]'s keyswitch scratch, grown as hexl_keyswitch grows it -- hexl_ks_scratch_bytes(plans[0],
 * batch) bytes, of which this call uses the first lane (min(batch, chunk) x (L*L + 4L + 4) x n doubles: 2.5 GiB of the 5.1 GiB at
 * n = 16384, L = 7, batch >= 256); the other plans' scratch is not touched and nothing else is allocated. The input-range flag
 * (hexl_ks_range_check) is raised on plans[0] only. */
int hexl_rotate_hoisted(hexl_ks_plan* const* plans, const uint64_t* galois_elts, size_t n_rot, uint64_t* const* d_outs,
                        const uint64_t* d_ct, size_t batch);
/* Linear transform ("double hoisting"): the whole loop rotate -> multiply_plain -> accumulate of the diagonal method in one call,
 *   d_out = sum_r pt_r . Rotate_{g_r}(ct) + pt_id . ct,
 * with the mod-up shared as in hexl_rotate_hoisted AND the mod-down shared: the plaintexts are also known modulo the special prime, so
 * they are multiplied in before the mod-down, the sum over the rotations is taken in the extended basis q_0 ... q_{L-1}, q_sp, and the
 * special-prime inverse and the mod-down run once -- L*L + 3L + 2 transforms per instance whatever n_rot is, against
 * (L*L + L) + n_rot (2L + 2) for hexl_rotate_hoisted. The n_rot rotated ciphertexts never exist in memory.
 *   plans[r], galois_elts[r]   as for hexl_rotate_hoisted, under the same matching rules (below)
 *   d_pts           HOST array of n_rot DEVICE pointers, each [L + 1][n]: row i < L is the plaintext modulo q_i, row L the plaintext
 *                   modulo the special prime (plan modulus K - 1); NTT form in the transforms' output order, every word below its
 *                   modulus; one plaintext serves every instance of the batch. When K = L + 1 this is exactly what
 *                   hexl_rns_ntt_fwd(plan, ..., count = 1, n_limbs = K) writes.
 *   d_pt_identity   NULL, or a device [L][n] plaintext for the un-rotated term pt_id . (c0, c1) -- the g = 1 diagonal, which needs no key
 *   d_ct, d_out     [batch][2][L][n]; d_out is WRITTEN
 * Per instance, every line modulo its limb's modulus and every output word canonical:
 *   u[d][slot]    = the keyswitch's mod-up of c1 (as above), slot = 0 ... L-1 and the special prime
 *   acc[k][slot]  = sum_r pt_r[slot] . ( sum_d sigma_{g_r}(u[d][slot]) . key_r[d][k][slot] )
 *   s'_k          = (INTT_sp(acc[k][sp]) + floor(q_sp / 2)) mod q_sp
 *   out[0][i]     = sum_r pt_r[i] . sigma_{g_r}(c0[i]) + pt_id[i] . c0[i] + (acc[0][i] - NTT_i((s'_0 + fix_i) mod q_i)) . msf_i
 *   out[1][i]     =                                      pt_id[i] . c1[i] + (acc[1][i] - NTT_i((s'_1 + fix_i) mod q_i)) . msf_i
 * sigma_g, fix_i and msf_i are those of hexl_rotate_hoisted; the pt_id terms are absent when d_pt_identity is NULL. With n_rot = 1, no
 * identity term and a plaintext whose every word is 1 the output is word for word hexl_rotate_hoisted's.
 * NOT word-identical to hexl_rotate_hoisted -> hexl_multiply_plain -> accumulate in general: that composition divides by q_sp and
 * rounds once per rotation and multiplies the rounded words, this call rounds the weighted sum once. The two differ by the plaintext-
 * weighted rounding terms, each below one unit per rotation before the weight; both decrypt to the same plaintext, this call with no
 * more noise (one rounding error instead of the sum of n_rot weighted ones).
 * Plans: all of one context, with the same n, L, K and moduli; FP64 plans only (every modulus < 2^52), n = 1024 ... 32768; every plan
 * with keys (else HEXL_E_NOKEYS); equal twiddles across the plans are the caller's responsibility. The same g, or the same plan, may
 * appear more than once.
 * HEXL_E_BADARG: a null pointer in the arguments or in plans / d_pts (d_pt_identity excepted), n_rot == 0, a plan that does not match
 * plans[0] or runs on the integer kernels, a g that is even or >= 2n, d_out overlapping d_ct, any d_pts[r] or d_pt_identity, a size
 * that overflows. batch == 0 returns 0 after these checks and writes nothing.
 * Asynchronous on the context's stream (one lane; the stream contract of hexl_ctx_set_stream holds as for any single launch); the
 * three host arrays may be reused as soon as the call returns. The input-range flag (hexl_ks_range_check) is raised on plans[0] for a
 * ciphertext word that is not below its modulus; plaintext words below their modulus are a precondition and are not flagged.
 * Device memory: plans[0]'s keyswitch scratch, grown and used as by hexl_rotate_hoisted (its multiply-accumulate output is the
 * accumulator), and n_rot x 16 bytes of the context's grow-only table space; nothing else is allocated. */
int hexl_linear_transform(hexl_ks_plan* const* plans, const uint64_t* galois_elts, const uint64_t* const* d_pts, size_t n_rot,
                          const uint64_t* d_pt_identity, uint64_t* d_out, const uint64_t* d_ct, size_t batch);
/* Baby-step/giant-step linear transform: the diagonal method for many diagonals in one call,
 *   d_out = sum_j Rotate_{G_j}( sum_i pt_{j,i} . Rotate_{g_i}(ct) + pt_id_j . ct ),
 * with n_baby + n_giant Galois keys and key multiply-accumulate passes instead of n_baby * n_giant: the mod-up of ct and the n_baby key
 * passes run once and their outputs are kept, every giant step weights and sums the kept products without touching a key, and only the
 * n_giant outer rotations run a keyswitch of their own.
 *   baby_plans[i], baby_elts[i]     i < n_baby: the switching key from s(X^g_i) to s and g_i, as for hexl_linear_transform
 *   giant_plans[j], giant_elts[j]   j < n_giant: the switching key from s(X^G_j) to s and G_j; giant_plans[j] may be NULL when G_j = 1
 *   d_pts           HOST array of n_giant * n_baby DEVICE pointers, row-major (j, i): NULL for an absent diagonal, else a [L + 1][n]
 *                   plaintext with the rows and the order of hexl_linear_transform's d_pts[r]. As in every baby-step/giant-step scheme
 *                   the caller supplies diagonal (j, i) already rotated by G_j^-1: this call applies Rotate_{G_j} to the whole inner sum.
 *   d_pt_identity   NULL, or a HOST array of n_giant entries, each NULL or a device [L][n] plaintext: the key-free baby step g = 1 of
 *                   giant step j
 *   d_ct, d_out     [batch][2][L][n]; d_out is WRITTEN (whatever it held)
 * The output is fixed by the entry points above. For every giant step j
 *   t_j = hexl_linear_transform(the baby plans, elements and plaintexts of row j that are not NULL, in the order of i,
 *                               d_pt_identity[j], ct)        -- a row with only an identity term: t_j = pt_id_j . (c0, c1) mod q_i
 *   r_j = t_j                                                    if G_j = 1
 *         hexl_rotate_hoisted(&giant_plans[j], &G_j, 1, ., t_j)  otherwise
 *   out = sum_j r_j mod q_i, every word canonical
 * and the call is word for word that composition: both building blocks end in canonical words that depend on exact residue classes
 * only, so neither the order of accumulation nor the fact that the baby products are stored rather than recomputed changes a word. As
 * for the two building blocks, these are NOT the words of a route through hexl_rotate (digits lifted after the permutation there,
 * before it here), nor of hexl_rotate_hoisted -> hexl_multiply_plain -> accumulate; all of them decrypt to the same plaintext.
 * Plans: every non-NULL plan, baby or giant, under hexl_linear_transform's matching rules -- one context, the same n, L, K and moduli,
 * FP64 plans only, n = 1024 ... 32768, equal twiddles the caller's responsibility. A baby plan may be NULL when no row has a plaintext
 * in its column. Every plan that is used (a baby plan whose column has a plaintext, a giant plan with G_j != 1) needs keys, else
 * HEXL_E_NOKEYS. The same g may serve as a baby and as a giant step, and a plan may appear more than once.
 * HEXL_E_BADARG: a null argument (d_pt_identity excepted; the arrays are looked at even when n_baby = 0), n_giant == 0, no plan at all
 * in the two arrays, a giant row with neither a plaintext nor an identity term, a non-NULL plan that does not match the first one or
 * runs on the integer kernels, a NULL baby plan whose column has a plaintext, a NULL giant plan with G_j != 1, an element that is even
 * or >= 2n (used or not), d_out overlapping d_ct, any plaintext or any identity plaintext, a size that overflows. n_baby == 0 is
 * allowed when every row has its identity term. batch == 0 returns 0 after these checks and writes nothing.
 * Asynchronous on the context's stream (one lane; the stream contract of hexl_ctx_set_stream holds as for any single launch); all host
 * arrays may be reused as soon as the call returns. The input-range flag (hexl_ks_range_check) is raised on the first non-NULL plan of
 * baby_plans, then of giant_plans -- baby_plans[0] whenever it is given -- for a word of d_ct that is not below its modulus.
 * Device memory, all of it on that same plan and grow-only: its keyswitch scratch as for hexl_rotate_hoisted; the baby store,
 * n_baby x chunk x 2 (L + 1) n doubles (2 MiB per baby step and instance at n = 16384, L = 7); one giant step's inner result, chunk x
 * 2 L n words. chunk = min(batch, the keyswitch's chunk), cut down so that the baby store stays within 2 GiB (never below one
 * instance; at n = 16384, L = 7 the full chunk of 256 up to 4 baby steps, 128 instances at 8, 64 at 16); HEXL_KS_CHUNK forces the
 * chunk whatever the store then takes. hexl_lt_bsgs_scratch_bytes(plan, n_baby, batch) is the sum of the three for a call with that
 * plan first (capacity planning, as hexl_ks_scratch_bytes). The context's grow-only table space takes 32 bytes per plaintext. */
int hexl_linear_transform_bsgs(hexl_ks_plan* const* baby_plans, const uint64_t* baby_elts, size_t n_baby,
                               hexl_ks_plan* const* giant_plans, const uint64_t* giant_elts, size_t n_giant,
                               const uint64_t* const* d_pts, const uint64_t* const* d_pt_identity, uint64_t* d_out,
                               const uint64_t* d_ct, size_t batch);
size_t hexl_lt_bsgs_scratch_bytes(const hexl_ks_plan* plan, size_t n_baby, size_t batch);
/* Domain changes and the plaintext product for ciphertexts that live on the device: the ends of a flow (encode / encrypt need the
 * forward transform, decrypt / decode the inverse) and the multiplier of a linear layer (rotate -> multiply_plain -> accumulate).
 * All three are asynchronous on the context's stream, need no keys and keep no device memory in the plan. FP64 plans only (every
 * modulus < 2^52) and n = 1024 ... 32768, as hexl_rescale; 1 <= n_limbs <= K: the moduli are the plan's first n_limbs, so a
 * ciphertext after rescales passes its smaller n_limbs, and n_limbs = K takes key material through the special prime as well.
 * Precondition: every input word is below its modulus. Every output word is canonical, in [0, q_i).
 *
 * RNS transforms: d_in, d_out [count][n_limbs][n], count = instances x components (a ciphertext batch passes batch * 2); polynomial
 * (c, i) is transformed modulo q_i with the plan's own tables (derived, or the h_twiddles given to hexl_ks_plan_create) in one launch.
 * Forward: negacyclic NTT, coefficients in natural order in, the transforms' bit-reversed order out -- the form every other entry
 * point takes. Inverse: the reverse, n^-1 included. Bit-exact with hexl_ntt_fwd / hexl_ntt_inv on tables of the same root.
 * d_out == d_in (in place) is allowed; any other overlap, a null pointer, n_limbs outside 1 ... K or a size that overflows:
 * HEXL_E_BADARG. count == 0 returns 0. */
int hexl_rns_ntt_fwd(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* d_in, size_t count, uint64_t n_limbs);
int hexl_rns_ntt_inv(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* d_in, size_t count, uint64_t n_limbs);
/* Plaintext multiply, everything in NTT form:
 *   d_ct, d_out [batch][n_components][n_limbs][n], d_pt [pt_batch][n_limbs][n], pt_batch = 1 (one plaintext for every instance) or batch
 *   out[b][k][i][j] = ct[b][k][i][j] * pt[b or 0][i][j] mod q_i, WRITTEN when accumulate == 0, else added to the word d_out holds
 *   (itself below q_i) mod q_i.
 * 1 <= n_components <= 3. d_out == d_ct is allowed when accumulate == 0; d_out must not overlap d_pt; every other overlap (d_out == d_ct
 * with accumulate != 0 among them), another pt_batch or a size that overflows: HEXL_E_BADARG. */
int hexl_multiply_plain(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* d_ct, const uint64_t* d_pt, size_t batch,
                        uint64_t n_components, uint64_t n_limbs, size_t pt_batch, int accumulate);
/* Weighted sum of up to eight ciphertexts, limb by limb, everything in NTT form: ct + ct, ct - ct, -ct, ct . constant, ct + plaintext,
 * ct + constant and the CKKS level drop are all this one call with special weights. For b < batch, k < n_components, i < n_limbs, j < n
 *   out[b][k][i][j] = ( sum_t w[t][i] . ct_t[b][k][i][j]  +  [k == 0] . (pt[b or 0][i][j] + const[i]) ) mod q_i, canonical.
 *   d_cts       HOST array of n_terms DEVICE pointers, 1 <= n_terms <= 8; term t is [batch][n_components][in_limbs[t]][n], every word
 *               below its modulus
 *   in_limbs    HOST [n_terms], n_limbs <= in_limbs[t] <= K, or NULL: every term has n_limbs. A term with more limbs than the output is
 *               read through its first n_limbs limbs only -- the CKKS level drop: the last moduli of the plan's chain are discarded, as
 *               hexl_rescale and hexl_rns_ntt_* do when they use "the plan's first n_limbs"
 *   h_weights   HOST [n_terms][n_limbs] residues, each below q_i, or NULL: every weight is 1. 1 adds the term, q_i - 1 subtracts it,
 *               rint(a . scale) mod q_i multiplies it by a scaled constant
 *   d_pt        NULL, or a DEVICE plaintext [pt_batch][n_limbs][n], words below q_i, added to component 0 only; pt_batch = 1 or batch as
 *               for hexl_multiply_plain, ignored when d_pt is NULL
 *   h_const     NULL, or HOST [n_limbs] residues below q_i, added to every word of component 0 (in NTT form a constant polynomial is the
 *               same word at every index)
 *   d_out       [batch][n_components][n_limbs][n], WRITTEN
 * 1 <= n_components <= 3, 1 <= n_limbs <= K; FP64 plans only, n = 1024 ... 32768, no keys needed, as hexl_multiply_plain. Every term is
 * read once and the output written once: n_terms + 1 passes over memory.
 * Overlap: d_out may be exactly d_cts[t] for terms with in_limbs[t] == n_limbs (a lane reads only the words it writes: in place, and
 * accumulation with d_out among the terms); terms may overlap each other and d_pt. Any other overlap of d_out with a term or with d_pt:
 * HEXL_E_BADARG.
 * HEXL_E_BADARG as well: a null plan, d_out, d_cts or d_cts[t] (batch == 0 does not excuse it), n_terms outside 1 ... 8, an in_limbs[t]
 * outside its range, a weight or a constant that is not below its modulus, another pt_batch, a plan on the integer kernels, a size or
 * a grid that overflows. batch == 0 returns 0 after these checks.
 * Asynchronous on the context's stream. Pointers, limb counts, weights and the constant travel in the kernel's arguments: every host
 * array may be reused as soon as the call returns, and the call allocates and keeps no device memory. */
int hexl_ct_lincomb(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* const* d_cts, const uint64_t* in_limbs,
                    const uint64_t* h_weights, size_t n_terms, const uint64_t* d_pt, size_t pt_batch,
                    const uint64_t* h_const, size_t batch, uint64_t n_components, uint64_t n_limbs);
/* Ciphertext x ciphertext with the relinearisation placed by the caller ("lazy relinearisation"). Relinearisation is linear, so a sum
 * of products needs ONE key switch -- L*L + 3L + 2 transforms per instance -- where hexl_multiply_relinearize per pair spends one per
 * term: inner products, ciphertext matrix products, the giant-step sums of a polynomial evaluation, "multiply now, relinearize after
 * the additions". Everything in NTT form.
 *
 * hexl_ct_tensor_sum: the sum of up to eight tensor products, three components out. For b < batch, i < n_limbs, j < n, modulo q_i,
 * every word canonical:
 *   out[b][0][i][j] = sum_t a_t[b][0][i][j] . b_t[b][0][i][j]
 *   out[b][1][i][j] = sum_t ( a_t[b][0][i][j] . b_t[b][1][i][j] + a_t[b][1][i][j] . b_t[b][0][i][j] )
 *   out[b][2][i][j] = sum_t a_t[b][1][i][j] . b_t[b][1][i][j]
 *   d_as, d_bs  HOST arrays of n_terms DEVICE pointers, 1 <= n_terms <= 8; a_t is [batch][2][in_limbs[2t]][n] and b_t is
 *               [batch][2][in_limbs[2t+1]][n], every word below its modulus. d_as[t] == d_bs[t] is allowed (a square); operands may
 *               overlap each other in any way
 *   in_limbs    HOST [n_terms][2], n_limbs <= in_limbs[.] <= K, or NULL: every operand has n_limbs. An operand with more limbs than the
 *               output is read through its first n_limbs limbs only -- the CKKS level drop: the last moduli of the plan's chain are
 *               discarded, as hexl_rescale and hexl_rns_ntt_* do when they use "the plan's first n_limbs"
 *   d_out       [batch][3][n_limbs][n], WRITTEN: what hexl_ct_lincomb, hexl_rescale and hexl_rlwe_decrypt take with n_components = 3.
 *               Sums of more than eight products are chained through hexl_ct_lincomb on three components
 * 1 <= n_limbs <= K; FP64 plans only, n = 1024 ... 32768, no keys needed, as hexl_ct_lincomb. Every operand is read once and the output
 * written once: 4 n_terms + 3 polynomial passes per limb.
 * HEXL_E_BADARG: a null plan, d_out, d_as, d_bs, d_as[t] or d_bs[t] (batch == 0 does not excuse it), n_terms outside 1 ... 8, an
 * in_limbs entry outside its range, a plan on the integer kernels, d_out overlapping any operand (the layouts differ: there is no
 * in-place form), a size or a grid that overflows. batch == 0 returns 0 after these checks.
 * Asynchronous on the context's stream. Pointers and limb counts travel in the kernel's arguments: every host array may be reused as
 * soon as the call returns, and the call allocates and keeps no device memory. */
int hexl_ct_tensor_sum(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* const* d_as, const uint64_t* const* d_bs,
                       const uint64_t* in_limbs, size_t n_terms, size_t batch, uint64_t n_limbs);
/* Relinearize: d_ct3[batch][3][L][n] -> d_out[batch][2][L][n] WRITTEN with (c0, c1) + KeySwitch(c2), i.e. what
 * hexl_keyswitch(result = components 0..1, t_target = component 2) leaves. The plan's keys must be the relinearisation key
 * (hexl_ks_gen_keys with HEXL_KEY_FROM_SQUARE; the caller's responsibility). Runs on every plan hexl_keyswitch accepts, integer kernels
 * included: the call moves words and runs the key switch, with no arithmetic of its own. Asynchronous on the context's stream.
 * HEXL_E_BADARG for a null pointer, d_out overlapping d_ct3 or a size that overflows; then HEXL_E_NOKEYS before hexl_ks_set_keys; then
 * batch == 0 returns 0. Device memory kept by the plan, grow-only, beside the keyswitch's scratch: min(batch, chunk) x L x n words
 * (component 2 of one slice) -- the very buffer hexl_rotate keeps for sigma_g(c1), shared between the two. */
int hexl_relinearize(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* d_ct3, size_t batch);
/* d_out[batch][2][L][n] WRITTEN with the relinearised sum of up to eight products: word for word
 *   hexl_ct_tensor_sum(plan, tmp, d_as, d_bs, in_limbs, n_terms, batch, n_limbs = L) followed by hexl_relinearize(plan, d_out, tmp, batch)
 * (both end in canonical words that depend on exact residues only) -- but the three-component sum never exists in memory: slice by
 * slice the tensor kernel writes components 0-1 into d_out and component 2 into the key switch's t_target slice. One key switch per
 * output ciphertext whatever n_terms is: (n_terms - 1) (L*L + 3L + 2) transforms per instance fewer than n_terms calls of
 * hexl_multiply_relinearize and a hexl_ct_lincomb. With n_terms = 1 the output is word for word hexl_multiply_relinearize's, which
 * serves one pair better (its product never leaves the chip).
 * d_as, d_bs, in_limbs, n_terms as for hexl_ct_tensor_sum with n_limbs = L: in_limbs entries in L ... K. FP64 plans only, n = 1024 ...
 * 32768. HEXL_E_BADARG as for hexl_ct_tensor_sum (d_out must not overlap any operand); then HEXL_E_NOKEYS; then batch == 0 returns 0.
 * Asynchronous on the context's stream; the host arrays may be reused as soon as the call returns. Device memory: hexl_relinearize's. */
int hexl_multiply_sum_relinearize(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* const* d_as, const uint64_t* const* d_bs,
                                  const uint64_t* in_limbs, size_t n_terms, size_t batch);
/* Encode and decode on the device: the canonical embedding and the change between real coefficients and RNS limbs, so that weights and
 * results can cross the bus as slot vectors (n/2 complex doubles) instead of [n_limbs][n] words. All four are asynchronous on the
 * context's stream and need no keys. FP64 plans only (every modulus < 2^52), n = 1024 ... 32768, 1 <= n_limbs <= K: the moduli are the
 * plan's first n_limbs, as for hexl_rns_ntt_fwd. The word side is [count][n_limbs][n] in NTT form, in the transforms' bit-reversed output
 * order: what hexl_rns_ntt_fwd writes and what hexl_multiply_plain and the d_pts of hexl_linear_transform read (n_limbs = K = L + 1).
 * zeta = exp(i pi / n); slot k < n/2 belongs to the evaluation point zeta^(5^k mod 2n) (SEAL's convention), so hexl_rotate with g = 5
 * moves slot k + 1 to slot k.
 *   hexl_rns_from_f64   d_coeffs double [count][n], real coefficients in natural order; out[c][i] = NTT_i(rint(coeff_j) mod q_i), every
 *                       word canonical. rint rounds to nearest, ties to even; a negative integer r maps to q_i - (|r| mod q_i), or 0.
 *                       Exact for every finite coefficient with |rint(c)| < 2^62 (doubles above 2^53 are reduced as the integers they
 *                       are). A coefficient outside that raises the plan's input-range flag (hexl_ks_range_check); the words of that
 *                       instance are then unspecified, nothing else is affected.
 *   hexl_rns_to_f64     the reverse: INTT_i of every limb, then per coefficient the CRT value x in (-Q/2, Q/2), Q = q_0 ... q_(n_limbs-1),
 *                       as a double: exact when |x| < 2^53, relative error at most 2^-50 otherwise. Precondition: every input word is
 *                       below its modulus.
 *   hexl_ckks_encode    d_slots double [count][n/2][2] (re, im); out = hexl_rns_from_f64 of
 *                       coeff_j = scale (2/n) Re(sum_k z_k zeta^(-j 5^k)), the real polynomial m with m(zeta^(5^k)) = scale z_k before
 *                       rounding. The range precondition and flag are those of hexl_rns_from_f64, on the scaled coefficients.
 *   hexl_ckks_decode    z_k = m(zeta^(5^k)) / scale with m's coefficients from hexl_rns_to_f64.
 * The transforms between slots and coefficients are FFTs in double on correctly rounded twiddles: the 2-norm error of a result is
 * within 16 log2(n) 2^-53 of its 2-norm.
 * HEXL_E_BADARG: a null pointer (count == 0 does not excuse it), a plan on the integer kernels, n_limbs outside 1 ... K, a scale that is
 * not finite and positive, a size that overflows, input and output ranges that overlap. count == 0 returns 0 after these checks.
 * Device memory, kept in the plan and grow-only: the real coefficients of one chunk (encode, decode: n doubles per instance) and its
 * coefficient-form limbs (rns_to_f64, decode: n_limbs x n words per instance); a chunk is 256 instances at n = 16384 and the same number
 * of coefficients at every other n. Tables made at first use: the 2n-th roots of unity (32 n bytes), the slot order (2 n bytes) and
 * Garner's constants (4 KiB). */
int hexl_rns_from_f64(hexl_ks_plan* plan, uint64_t* d_out, const double* d_coeffs, size_t count, uint64_t n_limbs);
int hexl_rns_to_f64(hexl_ks_plan* plan, double* d_coeffs, const uint64_t* d_in, size_t count, uint64_t n_limbs);
int hexl_ckks_encode(hexl_ks_plan* plan, uint64_t* d_out, const double* d_slots, size_t count, uint64_t n_limbs, double scale);
int hexl_ckks_decode(hexl_ks_plan* plan, double* d_slots, const uint64_t* d_in, size_t count, uint64_t n_limbs, double scale);
/* Sampling, symmetric encryption and decryption on the device: with them a flow starts from slot vectors and a 32-byte seed and ends in
 * slot vectors -- no ciphertext, error polynomial or mask crosses the bus, and the raw material of every switching key is one call.
 *
 * WARNING: (seed, stream, absolute polynomial index) MUST NEVER BE USED TWICE WITH ONE SECRET. The streams are deterministic: the same
 * triple gives the same mask `a` and the same error `e`, and two encryptions under one (a, e) reveal the difference of their plaintexts
 * (c0 - c0' = pt - pt'); an encryption and a hexl_sample call that share a triple publish the error. Give every call sequence of one
 * secret its own `stream` (or a fresh seed from the operating system's generator), and advance `first` by `count` between calls that
 * share both. Distinct kinds never collide (the kind is part of the block counter), distinct streams and distinct indices neither.
 * hexl_ks_gen_keys (below) is such a call: it consumes the UNIFORM and CBD21 polynomials first ... first + L - 1 of its (seed, stream),
 * exactly as the key-shaped hexl_rlwe_encrypt it replaces -- never give two keys of one secret the same triple.
 * hexl_hks_keygen (further below) is such a call as well: it consumes the UNIFORM and CBD21 polynomials first ... first + sum_r dnum_r - 1
 * of its (seed, stream), dnum_r per key in the order of its array -- advance `first` by that sum between calls that share both.
 * hexl_pk_encrypt is another: for every instance c = first + b it consumes the TERNARY polynomial c and the CBD21 polynomials 2c and
 * 2c + 1 of its (seed, stream). A (seed, stream) it uses must not be shared with hexl_sample, hexl_rlwe_encrypt or hexl_ks_gen_keys of
 * the same key material (their CBD21 index c is its index 2c' or 2c' + 1 for some c'), and `first` advances by `count` between calls.
 *
 * The streams (normative): ChaCha20 in counter mode, the 20-round block function of RFC 8439 on the state
 *   words 0-3 the constants 0x61707865 0x3320646e 0x79622d32 0x6b206574 | words 4-11 seed[0..7] (the caller's 32 bytes as eight
 *   little-endian u32) | words 12, 13 low and high half of ctr = (kind << 60) | block | words 14, 15 low and high half of `stream`;
 * output words w[0..15] (rounds + input state), u64 lane t < 8 = w[2t] | w[2t+1] << 32. c = first + local index is the ABSOLUTE
 * polynomial index, so neither the split of a batch into calls nor anything inside the library changes a word:
 *   HEXL_SAMPLE_UNIFORM  word j of polynomial (c, limb i): block = ((c 16 + i) n + j) >> 2, t = 2 (j & 3), r = lane[t] + 2^64 lane[t+1],
 *                        word = r mod q_i -- uniform below q_i up to a bias under 2^-76, and uniform words are a uniform polynomial
 *                        in NTT form as in coefficient form. The stream depends on i, not on n_limbs: the limbs of a lower level are
 *                        a prefix of those of a higher one.
 *   HEXL_SAMPLE_TERNARY  coefficient j of polynomial c, ONE integer polynomial shared by all limbs: block = (c n + j) >> 3,
 *                        r = lane[j & 7], v = ((r 3) >> 64) - 1 in {-1, 0, 1} (secrets)
 *   HEXL_SAMPLE_CBD21    the same addressing, v = popcount(r & 0x1FFFFF) - popcount((r >> 21) & 0x1FFFFF): |v| <= 21, sigma = sqrt(10.5)
 *                        (SEAL's centred binomial error)
 * A small value v becomes the words NTT_i(v mod q_i), negative v as q_i - |v|: what hexl_rns_from_f64 makes of the double v.
 *
 *   hexl_sample         d_out [count][n_limbs][n] WRITTEN with polynomials first ... first + count - 1 of the stream (seed, stream, kind),
 *                       NTT form, canonical words.
 *   hexl_rlwe_encrypt   d_out [count][2][n_limbs][n] WRITTEN with (pt + e - a s, a): a = the UNIFORM and e = the CBD21 polynomial
 *                       first + b of (seed, stream). d_pt NULL (an encryption of zero: a public key, the mask of a key-switching
 *                       key) or [pt_batch][n_limbs][n] in NTT form (hexl_ckks_encode's output), pt_batch = 1 or count, ignored when d_pt
 *                       is NULL. d_secret [>= n_limbs][n]: NTT_i(s) in the plan's first n_limbs limbs, one secret for all instances (rows
 *                       beyond n_limbs are not read: a secret kept at K limbs serves every level). Word for word the composition
 *                       hexl_sample(UNIFORM), hexl_sample(CBD21), hexl_multiply_plain, hexl_ct_lincomb. Component 1 is a function of
 *                       the seed: a sender may ship (c0, seed, stream, first) and the receiver expand `a` with hexl_sample.
 *   hexl_rlwe_decrypt   d_out [count][n_limbs][n] WRITTEN with c0 + c1 s (+ c2 s^2 when n_components = 3) mod q_i, evaluated by
 *                       Horner; d_ct [count][n_components][n_limbs][n], n_components 2 or 3 (3: a product before relinearisation);
 *                       d_secret as above. The result is the plaintext plus the noise: hexl_ckks_decode takes it as it is.
 *   hexl_pk_encrypt     encryption under a public key, fused. d_out [count][2][n_limbs][n] WRITTEN: for instance b, c = first + b,
 *                         out[b][0] = pk0 u_c + e0_c + pt      out[b][1] = pk1 u_c + e1_c      modulo q_i, canonical words,
 *                       u_c = the TERNARY polynomial c, e0_c and e1_c = the CBD21 polynomials 2c and 2c + 1 of (seed, stream), each
 *                       entering as NTT_i(v mod q_i) as hexl_sample makes it. d_pk [2][pk_limbs][n] in NTT form, every word below its
 *                       modulus, n_limbs <= pk_limbs <= K: (pk0, pk1) = (e - a s, a), exactly what hexl_rlwe_encrypt(d_pt = NULL,
 *                       count = 1, n_limbs = pk_limbs) writes. Only the first n_limbs limbs of each component are read (the component
 *                       stride is pk_limbs n): a key kept at K limbs serves every level. d_pt NULL (an encryption of zero, for
 *                       re-randomisation) or [pt_batch][n_limbs][n], pt_batch = 1 or count, as for hexl_rlwe_encrypt. No secret is needed.
 *                       Normative definition: word for word the composition
 *                         U = hexl_sample(TERNARY, first, count);  E = hexl_sample(CBD21, 2 first, 2 count) viewed as [count][2][n_limbs][n];
 *                         T = hexl_multiply_plain(ct = the key's first n_limbs limbs replicated per instance, pt = U, n_components = 2,
 *                         pt_batch = count);  d_out = hexl_ct_lincomb(terms {T, E}, d_pt, pt_batch)
 *                       -- four launches and a key-sized replica per instance, which this call replaces by the sampling launches and
 *                       ONE combine kernel (four polynomial reads and two writes per instance and limb, the key from cache).
 * Key-shaped output: hexl_rlwe_encrypt with count = L (decomp_modulus_size), n_limbs = K, pt_batch = count writes [L][2][K][n] --
 * word for word the h_keys layout of hexl_ks_set_keys (key d at d 2 K n, word (k K + i) n + j). With
 *   pt[d][i] = [i == d] (P mod q_i) s'_i     P = the special prime, the plan's modulus K - 1; s' = the key being switched FROM
 * (s^2 for relinearisation, s(X^g) for the Galois key of g), the output is a switching key from s' to s: pt is L calls of
 * hexl_ct_lincomb on NTT(s') with per-limb weights. hexl_ks_set_keys_device (below) installs such a device buffer into a plan as it
 * is, and hexl_ks_gen_keys writes that very key straight into the plan without the buffer ever existing: no key has to cross the bus
 * (a download and hexl_ks_set_keys remain the way to keep a copy on the host). Public-key encryption is hexl_pk_encrypt on a public key
 * made here with d_pt = NULL and count = 1.
 * Common rules: FP64 plans only (every modulus < 2^52), n = 1024 ... 32768, 1 <= n_limbs <= K (the plan's first n_limbs moduli), no keys
 * needed. Asynchronous on the context's stream; the seed travels by value in the kernels' arguments, so every host array may be
 * reused as soon as the call returns. Precondition: every input word is below its modulus. Every output word is canonical.
 * HEXL_E_BADARG: a null plan, output, seed, secret or (decrypt) ciphertext -- count == 0 does not excuse it --, an unknown kind, a plan
 * on the integer kernels, n_limbs outside 1 ... K, pt_batch other than 1 or count when d_pt is given, n_components outside {2, 3},
 * first + count > 2^40 (this keeps every block index below 2^60), a size or a grid that overflows, any overlap of the output with an
 * input. count == 0 returns 0 after these checks and writes nothing. hexl_pk_encrypt: the same list with the key in the secret's place,
 * and pk_limbs outside n_limbs ... K, first + count > 2^39 (this keeps the CBD21 indices 2c + 1 below 2^40), any overlap of d_out with
 * the key's full [2][pk_limbs][n] extent or with d_pt.
 * Device memory, kept in the plan and grow-only, shared with encode / decode: the small kinds and the error of an encryption pass
 * through one chunk of real coefficients (n doubles per instance), hexl_rlwe_encrypt also through the chunk's NTT-form error
 * (n_limbs x n words per instance); a chunk is 256 instances at n = 16384 and the same number of coefficients at every other n.
 * hexl_pk_encrypt passes the mask and the two errors of an instance through the same two buffers (3 n doubles and 3 x n_limbs x n
 * words per instance) in chunks of a third of that -- 85 instances at n = 16384, 1365 at n = 1024 --, so it never holds more than a full
 * chunk of hexl_rlwe_encrypt does (32 MiB + n_limbs x 32 MiB). UNIFORM and hexl_rlwe_decrypt are one launch and keep nothing. */
#define HEXL_SAMPLE_UNIFORM 1
#define HEXL_SAMPLE_TERNARY 2
#define HEXL_SAMPLE_CBD21   3
int hexl_sample(hexl_ks_plan* plan, uint64_t* d_out, int kind, const uint32_t seed[8], uint64_t stream, uint64_t first,
                size_t count, uint64_t n_limbs);
int hexl_rlwe_encrypt(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* d_pt, size_t pt_batch, const uint64_t* d_secret,
                      const uint32_t seed[8], uint64_t stream, uint64_t first, size_t count, uint64_t n_limbs);
int hexl_pk_encrypt(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* d_pt, size_t pt_batch, const uint64_t* d_pk, uint64_t pk_limbs,
                    const uint32_t seed[8], uint64_t stream, uint64_t first, size_t count, uint64_t n_limbs);
int hexl_rlwe_decrypt(hexl_ks_plan* plan, uint64_t* d_out, const uint64_t* d_ct, const uint64_t* d_secret, size_t count,
                      uint64_t n_components, uint64_t n_limbs);
/* Switching keys without a host round trip. Keys are per plan, and plans are per level and per Galois element: a rotation set keys every
 * one of its plans with one asynchronous call each, and neither a secret nor a key leaves the device.
 *
 * hexl_ks_set_keys_device: hexl_ks_set_keys for keys that are on the device already.
 *   d_keys: DEVICE [L][2][K][n] in the h_keys layout of hexl_ks_set_keys (key d at d*2*K*n, word (k*K + i)*n + j) -- what a key-shaped
 *   hexl_rlwe_encrypt writes. Afterwards the plan is word for word the plan hexl_ks_set_keys leaves for the same words.
 * Runs on every plan hexl_ks_set_keys accepts, integer-kernel plans included. Any 64-bit word is taken and reduced modulo its limb's
 * modulus, as on the host; only limbs i < L and i = K - 1 are read, as on the host. One kernel on the context's stream reads the
 * caller's buffer once and writes every copy of the keys the plan holds (centred doubles in the order of each FP64 pipeline; words
 * beside their Shoup factors for the integer kernels): no host synchronisation, no host staging, no key-sized temporary and no device
 * memory beyond what hexl_ks_plan_create reserved. d_keys may be reused as soon as the kernel has run (stream order).
 * Ordering: every keyswitch-family call (hexl_keyswitch, hexl_multiply_relinearize, hexl_rotate, the hoisted and linear-transform calls)
 * joins the auxiliary lanes it used back into the context's stream before it returns, so this launch is behind every reader of the
 * old keys queued so far and in front of every reader of the new ones queued later. Re-keying a plan that is in use is therefore
 * allowed, with no synchronisation: install, launch, install, launch. (hexl_ks_set_keys synchronises the stream instead.)
 * HEXL_E_BADARG: a null plan or pointer; the plan is left as it was.
 *
 * hexl_ks_gen_keys: the switching key from s' to s, generated into the plan. Normative definition: afterwards the plan is word for word
 * what hexl_ks_set_keys leaves for the output of
 *   hexl_rlwe_encrypt(count = L, n_limbs = K, pt_batch = L, pt[d][i] = [i == d] (P mod q_i) s'_i, d_secret, seed, stream, first),
 * P = the plan's modulus K - 1, with
 *   HEXL_KEY_FROM_POLY     s' = d_from [K][n], NTT form
 *   HEXL_KEY_FROM_SQUARE   s'_i = s_i . s_i mod q_i: the relinearisation key (hexl_multiply_relinearize)
 *   HEXL_KEY_FROM_GALOIS   s'_i = the hexl_apply_galois permutation of s_i for galois_elt: the key hexl_rotate and the hoisted family
 *                          need for that element
 * d_secret is [K][n]: NTT_i(s) at ALL K limbs (hexl_sample(TERNARY, n_limbs = K)), every word below its modulus. galois_elt and d_from are
 * ignored where the kind does not use them. The call consumes polynomial indices first ... first + L - 1 of the UNIFORM and CBD21 kinds
 * of (seed, stream): see the WARNING above. Limbs the plan never reads (L <= i < K - 1 when K > L + 1) are skipped; the streams are
 * addressed by (polynomial, limb, index), so skipping changes no word.
 * FP64 plans only (every modulus < 2^52), n = 1024 ... 32768, as hexl_rlwe_encrypt. Asynchronous on the context's stream and ordered
 * like hexl_ks_set_keys_device; the seed travels by value. Fused: the CBD21 errors of the L keys pass through the plan's encode scratch
 * as in hexl_rlwe_encrypt, then ONE kernel reads e and s (s' only in the L rows whose plaintext is not zero -- gathered through the
 * Galois index or squared in registers), draws `a`, forms the canonical c0 = pt + e - a s and stores c0 and `a` as centred doubles at
 * their place in every copy of the keys. No [L][2][K][n] buffer, no plaintext, no s^2 and no s(X^g) exists in memory.
 * Device memory, kept in the plan and grow-only, shared with encode / decode / encrypt: L x n doubles and L x K x n words of the encode
 * scratch (1.9 MiB + 15 MiB at n = 16384, L = 7, K = 8); nothing else is allocated (a first call that grows them waits for the device).
 * HEXL_E_BADARG: a null plan, secret or seed; d_from null with HEXL_KEY_FROM_POLY; an unknown from_kind; HEXL_KEY_FROM_GALOIS with a
 * galois_elt that is even or >= 2n; first + L > 2^40; a plan on the integer kernels. A refused call leaves the plan as it was (without
 * keys, if it had none: HEXL_E_NOKEYS from hexl_keyswitch). */
int hexl_ks_set_keys_device(hexl_ks_plan* plan, const uint64_t* d_keys);
#define HEXL_KEY_FROM_POLY   0   /* s' = d_from [K][n], NTT form */
#define HEXL_KEY_FROM_SQUARE 1   /* s' = s^2: the relinearisation key */
#define HEXL_KEY_FROM_GALOIS 2   /* s' = s(X^galois_elt): the key hexl_rotate / the hoisted family need for that element */
int hexl_ks_gen_keys(hexl_ks_plan* plan, const uint64_t* d_secret, int from_kind, uint64_t galois_elt, const uint64_t* d_from,
                     const uint32_t seed[8], uint64_t stream, uint64_t first);
/* Hybrid key switching: digit groups and several special primes. Every key switch above is the per-limb gadget: each
 * of the L data limbs is a digit of its own and the plan's modulus K - 1 is the one special prime -- L*L + 3L + 2 transforms per
 * instance, L*2*(L + 1)*n key words per key, and a second plan with a second key for every lower level. The hybrid gadget groups alpha
 * limbs into one digit, uses n_p = K - L special primes and switches through ONE installed key at every level:
 *   L + sum_d (L + n_p - |G_d|) + 2 n_p + 2L transforms at the full level (L = 12, alpha = 4, n_p = 4: 80 against 182), dnum*2*K*n key
 *   words per key (96 n against 312 n).
 *
 * hexl_hks is attached to an FP64 plan (every modulus < 2^52, n = 1024 ... 32768) created with decomp_modulus_size = L data limbs and
 * key_modulus_size = K > L: limbs L ... K - 1 are the special primes S, P their product. It borrows the plan's context, stream, moduli
 * and tables -- destroy it BEFORE the plan -- and owns its keys, conversion constants and scratch. The plan itself is not changed:
 * hexl_keyswitch and every other entry point run on it as before, with the plan's own keys.
 *   digit_limbs = alpha, 1 <= alpha <= L; dnum = ceil(L / alpha); digit d covers the limbs G_d = {d alpha ... min((d + 1) alpha, L) - 1}
 *   d_keys      DEVICE [dnum][2][K][n]: key d at d*2*K*n, word (k*K + i)*n + j -- the h_keys layout of hexl_ks_set_keys with dnum in
 *               place of L. ALL K limbs are read. Precondition: NTT form, every word below its modulus. The plaintext of key d is
 *               P [i in G_d] s' modulo q_i and 0 modulo the special primes, whatever the level: one key serves every level.
 *               The install is one kernel on the context's stream, no host synchronisation, ordered like hexl_ks_set_keys_device:
 *               install, launch, install, launch re-keys an object in use. d_keys may be reused once the kernel has run (stream order).
 *   n_limbs = l, 1 <= l <= L: the level. d_t_target [batch][l][n]; d_result, d_out, d_ct [batch][2][l][n]; d_ct3 [batch][3][l][n]. At
 *               level l the digits are G_d restricted to the limbs below l, d < ceil(l / alpha) (the last one may be partial), and the
 *               basis is T_l = {0 ... l - 1} and S.
 * Per instance, every line modulo its limb's modulus and every stored word canonical (normative):
 *   1  a_i = INTT_i(t[i]) for i < l, in [0, q_i)
 *   2  mod-up by fast base conversion, no correction term. For digit d, D = the product of q_i over the digit's limbs at level l:
 *        y_i = a_i . ((D / q_i)^-1 mod q_i)
 *        x_d[j] = sum_i y_i . ((D / q_i) mod q_j),  ext_d[j] = NTT_j(x_d[j])   for every j of T_l outside the digit
 *        ext_d[j] = t[j]                                                          for j inside it
 *      (x_d is a lift of the digit in [0, |G_d| D))
 *   3  acc[k][j] = sum_d ext_d[j] . key[d][k][j]   for k in {0, 1}, j in T_l
 *   4  mod-down with rounding: for s in S   b_s = (INTT_s(acc[k][s]) + (floor(P / 2) mod q_s)),  z_s = b_s . ((P / q_s)^-1 mod q_s);
 *      for i < l   w_i = sum_s z_s . ((P / q_s) mod q_i)  and
 *        out[k][i] = result[k][i] + (acc[k][i] - NTT_i((w_i + fix_i) mod q_i)) . (P^-1 mod q_i),  fix_i = q_i - (floor(P / 2) mod q_i)
 * With alpha = 1 and K = L + 1 this is, term for term, the key switch of hexl_rotate_hoisted's description above, and d_keys is the
 * hexl_ks_set_keys_device layout: hexl_hks_keyswitch at n_limbs = L then equals hexl_keyswitch on the same plan and the same device key
 * buffer word for word (for a plan whose h_modswitch[i] is P^-1 mod q_i).
 *   hexl_hks_keyswitch    adds the key switch of d_t_target into d_result modulo q_i, exactly as hexl_keyswitch does
 *   hexl_hks_relinearize  d_out WRITTEN with (c0, c1) + KS(c2)
 *   hexl_hks_rotate       d_out WRITTEN with (sigma_g(c0), 0) + KS(sigma_g(c1)), sigma_g the permutation of hexl_apply_galois
 * All three are asynchronous on the context's stream, on one lane: the stream contract of hexl_ctx_set_stream holds as for any single
 * launch. Precondition: every input word is below its modulus. This version does NOT raise the input-range flag (hexl_ks_range_check):
 * the output words of an instance with an out-of-range word are unspecified and nothing reports it.
 * Noise: the switched ciphertext decrypts to t . s' plus an error of infinity norm at most
 *   21 n sum_d |G_d| D_d / P + (n_p + 1/2)(n + 1)     for CBD21 key errors and a ternary secret.
 * P >= max_d D_d keeps the first term near 21 n alpha dnum; that choice of special primes is the caller's and is NOT checked.
 * HEXL_E_BADARG: a null handle or pointer (batch == 0 does not excuse it), a plan on the integer kernels or with K = L, alpha outside
 * 1 ... L, n_limbs outside 1 ... L, a galois_elt that is even or >= 2n, an output that overlaps an input, a size or a grid that
 * overflows; then HEXL_E_NOKEYS before hexl_hks_set_keys_device; then batch == 0 returns 0.
 * Device memory, owned by the object: the keys (dnum*2*K*n doubles), 148 KiB of constants for all levels (computed at create time: 8 KiB of
 * source inverses and 128 KiB of target weights for the 32 base conversions -- 16 mod-ups, the mod-down, 15 rescaling mod-downs of the
 * hybrid multiply below -- and 12 KiB of per-limb constants of their 16 divisors), and
 * grow-only scratch for one chunk of min(batch, chunk) instances, chunk as for hexl_keyswitch (256 at n = 16384, the same number of
 * coefficients at other n; HEXL_KS_CHUNK): per instance L*n coefficient words, dnum*K*n extended doubles and 2*K*n accumulator doubles.
 * hexl_hks_scratch_bytes(hks, batch) is that sum at the full level (a lower level uses less of it). hexl_hks_relinearize and
 * hexl_hks_rotate keep one more grow-only buffer, the key switch's input of one slice: min(batch, chunk) x L x n words. */
typedef struct hexl_hks hexl_hks;
int hexl_hks_create(hexl_ks_plan* plan, uint64_t digit_limbs /* alpha */, hexl_hks** out);
int hexl_hks_destroy(hexl_hks* hks);                 /* before the plan it borrows */
int hexl_hks_set_keys_device(hexl_hks* hks, const uint64_t* d_keys);   /* DEVICE [dnum][2][K][n] */
int hexl_hks_keyswitch(hexl_hks* hks, uint64_t* d_result, const uint64_t* d_t_target, size_t batch, uint64_t n_limbs);
int hexl_hks_relinearize(hexl_hks* hks, uint64_t* d_out, const uint64_t* d_ct3, size_t batch, uint64_t n_limbs);
int hexl_hks_rotate(hexl_hks* hks, uint64_t* d_out, const uint64_t* d_ct, size_t batch, uint64_t n_limbs, uint64_t galois_elt);
size_t hexl_hks_scratch_bytes(const hexl_hks* hks, size_t batch);
/* Hybrid keys made and read on the device.
 *
 * hexl_hks_keygen: one switching key per object, generated into the objects; key r switches from s'_r to s. Normative definition:
 * afterwards object r is word for word what hexl_hks_set_keys_device leaves for the output of the Python wrapper
 *   plan.gen_hybrid_key(out, secret, alpha_r, s'_r, seed, stream, first_r),   first_r = first + sum of dnum_r' over r' < r,
 * that is, row (r, d) = (pt + e - a s, a) modulo all K limbs with a = the UNIFORM and e = the CBD21 polynomial first_r + d of
 * (seed, stream), pt_i = (P mod q_i) s'_(r,i) for i in G_d and 0 at every other limb, the special primes included, P = the product of
 * the plan's moduli L ... K - 1, and s'_r selected by from_kinds[r] with the constants and meanings of hexl_ks_gen_keys:
 *   HEXL_KEY_FROM_POLY     s'_r = d_froms[r] [K][n], NTT form, every word below its modulus
 *   HEXL_KEY_FROM_SQUARE   s'_(r,i) = s_i . s_i mod q_i: the key of hexl_hks_relinearize and the hybrid multiply
 *   HEXL_KEY_FROM_GALOIS   s'_(r,i) = the hexl_apply_galois permutation of s_i for galois_elts[r]: the key of hexl_hks_rotate and the hoisted
 *                          and BSGS calls for that element
 * Every step is exact modular arithmetic, so "word for word" is well defined. d_secret is [K][n]: NTT_i(s) at ALL K limbs, every word
 * below its modulus. galois_elts and d_froms may be NULL when no key's kind uses them; their entries for keys of other kinds are ignored.
 * All objects are attached to ONE plan; they may have different alpha (the prefix sum above is what makes that work). The same object
 * twice in one call is refused. n_keys <= HEXL_HKS_KEYGEN_MAX_KEYS = 64; a larger set takes several calls with `first` advanced by the
 * rows of the calls before -- the words depend on (seed, stream, first_r + d) alone, never on the split.
 * The call consumes polynomial indices first ... first + sum_r dnum_r - 1 of the UNIFORM and CBD21 kinds of (seed, stream): see the
 * WARNING at hexl_sample. Asynchronous on the context's stream and ordered like hexl_hks_set_keys_device: generate, launch, generate,
 * launch re-keys an object in use. The seed travels by value.
 * Fused: the CBD21 errors of all sum_r dnum_r rows pass through the plan's encode scratch as in hexl_rlwe_encrypt (in chunks of 256 rows
 * at n = 16384, the same number of coefficients at other n), then per chunk ONE kernel reads e and s (s' only in the rows i in G_d, whose
 * plaintext is not zero -- read, squared in registers or gathered through the Galois index), draws `a`, forms c0 = pt + e - a s and
 * stores c0 and `a` as centred doubles at their place in the object's keys. No [dnum][2][K][n] word buffer, no plaintext, no s^2 and no
 * s(X^g) exists in memory; nothing key-sized is allocated (the encode scratch is the plan's, grow-only: a first call that grows it waits
 * for the device).
 * Everything is validated before anything is launched, and a refused call leaves every object as it was (without keys, if it had none:
 * HEXL_E_NOKEYS from its callers). HEXL_E_BADARG: a null array, object, secret or seed; n_keys == 0 or above the limit; an unknown kind;
 * HEXL_KEY_FROM_POLY with a null d_froms or a null entry; HEXL_KEY_FROM_GALOIS with a null galois_elts or an element that is even or >= 2n;
 * objects on different plans; a repeated object; first + sum_r dnum_r > 2^40.
 *
 * hexl_hks_export_keys: the installed key as canonical words, the inverse of the install -- d_out [dnum][2][K][n] in the
 * hexl_hks_set_keys_device layout, every word in [0, q_i). One kernel on the context's stream. hexl_hks_set_keys_device(X) then export
 * gives X mod q exactly; export then hexl_hks_set_keys_device on another object of the same shape gives an identical object.
 * HEXL_E_BADARG: a null handle or pointer; then HEXL_E_NOKEYS before any key is installed or generated (nothing is written). */
#define HEXL_HKS_KEYGEN_MAX_KEYS 64
int hexl_hks_keygen(hexl_hks* const* hks, size_t n_keys, const int* from_kinds, const uint64_t* galois_elts,
                    const uint64_t* const* d_froms, const uint64_t* d_secret, const uint32_t seed[8], uint64_t stream, uint64_t first);
int hexl_hks_export_keys(const hexl_hks* hks, uint64_t* d_out);   /* DEVICE [dnum][2][K][n] WRITTEN, canonical words */
/* Hoisted rotations and the linear transform on the hybrid key switch: many plaintext-weighted rotations of ONE
 * ciphertext batch. R calls of hexl_hks_rotate repeat steps 1-2 of the definition above -- the l inverse transforms, the base
 * conversion and the sum_d (l + n_p - |G_d|) forward transforms -- which depend on c1 alone and not on the key. Per instance at the
 * full level of L = 12, alpha = 4, n_p = 4: 80 R transforms for R calls of hexl_hks_rotate, 48 + 32 R for hexl_hks_rotate_hoisted
 * (steps 1-2 once), 80 whatever R is for hexl_hks_linear_transform (step 4 once as well).
 *   hks[r]        the hybrid key from s(X^g_r) to s, galois_elts[r] = g_r; r < n_rot. All objects must be attached to the SAME plan with
 *                 the same alpha (an object owns its key and borrows everything else, so several objects on one plan is the natural
 *                 arrangement). The same object, or the same g, may appear more than once. hks[0]'s scratch is used; the other objects
 *                 contribute their keys only.
 *   n_limbs = l   the level, 1 <= l <= L. d_ct, d_out and d_outs[r] are DEVICE [batch][2][l][n]; d_outs is a HOST array of device pointers.
 *   d_pts         HOST array of n_rot device pointers, each [K][n]: the plaintext modulo ALL K plan limbs, in NTT form, every word below
 *                 its modulus -- exactly what hexl_rns_ntt_fwd or hexl_ckks_encode with n_limbs = K writes. Only the rows of T_l (i < l
 *                 and L ... K - 1) are read, so one encoded plaintext serves every level, as one key does.
 *   d_pt_identity NULL, or DEVICE [>= l][n] of which rows i < l are read: it weights the key-free term pt_id . (c0, c1).
 * Per instance, every line modulo its limb's modulus and every stored word canonical (normative). Let ext_d[j], j in T_l,
 * d < ceil(l / alpha), be steps 1-2 of the definition above applied to t = c1 (the rows inside their own digit, ext_d[j] = c1[j],
 * included), and sigma_g the word permutation of hexl_apply_galois.
 *   hexl_hks_rotate_hoisted, for every r:
 *     acc_r[k][j] = sum_d sigma_{g_r}(ext_d[j]) . key_r[d][k][j]
 *     d_outs[r] WRITTEN with step 4 applied to acc_r with result = (sigma_{g_r}(c0), 0)
 *   hexl_hks_linear_transform:
 *     acc[k][j] = sum_r pt_r[j] . (sum_d sigma_{g_r}(ext_d[j]) . key_r[d][k][j])   for j in T_l; step 4 applied ONCE to acc; d_out WRITTEN with
 *     out[0][i] = sum_r pt_r[i] . sigma_{g_r}(c0[i]) + pt_id[i] . c0[i] + down(acc[0])[i]
 *     out[1][i] =                                      pt_id[i] . c1[i] + down(acc[1])[i]
 *     down(acc)[i] = (acc[i] - NTT_i((w_i + fix_i) mod q_i)) . (P^-1 mod q_i) as in step 4; the pt_id terms are absent when d_pt_identity is NULL.
 * Every output word is the canonical residue of an exactly defined class: neither the order of accumulation nor where the c0 term is
 * added can change a word. Word identities (tested):
 *   - for g = 1 hexl_hks_rotate_hoisted is word for word hexl_hks_rotate;
 *   - for g != 1 it is NOT word for word hexl_hks_rotate -- the situation of hexl_rotate_hoisted against hexl_rotate: sigma_g applied to
 *     the extended digit negates coefficients, and the lifts of a negated coefficient differ by |G_d| D modulo q_j. Both are lifts of
 *     magnitude below |G_d| D_d congruent to the digit, and both decrypt alike under the same noise bound as above;
 *   - hexl_hks_linear_transform with n_rot = 1, no identity term and an all-ones plaintext is word for word hexl_hks_rotate_hoisted;
 *   - with alpha = 1, K = L + 1 and n_limbs = L both calls equal hexl_rotate_hoisted / hexl_linear_transform word for word on per-limb
 *     plans (h_modswitch[i] = P^-1 mod q_i) that got the same key buffers through hexl_ks_set_keys_device; the d_pts layouts coincide
 *     ([K][n] is [L + 1][n]).
 * Noise of the linear transform, for CBD21 key errors, a ternary secret and plaintexts given as small integer polynomials (the same
 * polynomial reduced modulo every limb of T_l, special primes included), ||.||_1 the 1-norm of the centred coefficient vector:
 *   (sum_r ||pt_r||_1) . 21 n sum_d |G_d| D_d / P + (n_p + 1/2)(n + 1)      -- the rounding term once; the identity term adds none.
 * HEXL_E_BADARG, in this order: a null argument or array entry, d_pt_identity excepted (batch == 0 does not excuse it); objects that do
 * not share hks[0]'s plan and alpha; n_limbs outside 1 ... L; a g that is even or >= 2n; an output that overlaps d_ct, another output,
 * any plaintext or the identity plaintext; a size or a grid that overflows; n_rot == 0 in the linear transform. Then HEXL_E_NOKEYS if
 * any object has no keys. Then 0 with nothing written for batch == 0, or for n_rot == 0 in hexl_hks_rotate_hoisted (which then checks
 * the three array arguments and d_ct for NULL only).
 * Both calls are asynchronous on the context's stream, on one lane; the host arrays may be reused on return (per-rotation pointers
 * travel in kernel arguments and in the context's grow-only table space). Precondition: every input word is below its modulus. This
 * version does NOT raise the input-range flag (hexl_ks_range_check) for them either.
 * Device memory: hks[0]'s scratch as above plus one grow-only buffer, min(batch, chunk) x L x n doubles -- in a plain key switch the
 * mod-down's w of component 1 overwrites the extended digits, which here must survive for the next rotation.
 * hexl_hks_hoisted_scratch_bytes(hks, batch) is hexl_hks_scratch_bytes plus that buffer; hexl_hks_scratch_bytes itself is unchanged. */
int hexl_hks_rotate_hoisted(hexl_hks* const* hks, const uint64_t* galois_elts, size_t n_rot, uint64_t* const* d_outs, const uint64_t* d_ct, size_t batch, uint64_t n_limbs);
int hexl_hks_linear_transform(hexl_hks* const* hks, const uint64_t* galois_elts, const uint64_t* const* d_pts, size_t n_rot, const uint64_t* d_pt_identity, uint64_t* d_out, const uint64_t* d_ct, size_t batch, uint64_t n_limbs);
size_t hexl_hks_hoisted_scratch_bytes(const hexl_hks* hks, size_t batch);
/* Baby-step/giant-step diagonals on the hybrid key switch, hexl_linear_transform_bsgs with the hybrid calls'
 * conventions:
 *   d_out = sum_j Rot_{G_j}( sum_i pt_{j,i} . Rot_{g_i}(ct) + pt_id_j . ct )   at level l = n_limbs
 * with n_baby + #{G_j != 1} hybrid keys and key passes instead of the n_baby x n_giant of one flat hexl_hks_linear_transform.
 *   baby_hks[i]   the hybrid key from s(X^g_i) to s, baby_elts[i] = g_i; i < n_baby. An entry may be NULL when no row has a plaintext in
 *                 its column.
 *   giant_hks[j]  the same for giant_elts[j] = G_j; j < n_giant. May be NULL when G_j = 1.
 *                 Every non-NULL object must be attached to the SAME plan with the same alpha. Objects and elements may repeat, and one
 *                 g may be a baby step and a giant step. The first non-NULL object (baby array first, then giant) owns the scratch, as
 *                 hks[0] does above; the others contribute their keys only.
 *   d_pts         HOST array of n_giant x n_baby DEVICE pointers, row-major (j, i). NULL = an absent diagonal; otherwise [K][n] exactly as
 *                 for hexl_hks_linear_transform (all K plan limbs, NTT form, only the rows of T_l read: one encoded plaintext serves every
 *                 level). Diagonal (j, i) is supplied already rotated by G_j^-1.
 *   d_pt_identity NULL, or a HOST array of n_giant entries, each NULL or DEVICE [>= l][n].
 *   d_ct, d_out   DEVICE [batch][2][l][n]; d_out is WRITTEN.
 * Definition (normative): the composition of the two calls above. For every giant step j
 *   t_j = hexl_hks_linear_transform(row j's non-NULL baby objects, elements and plaintexts in the order of i, d_pt_identity[j], ct, l)
 *         (a row with only an identity term: t_j = pt_id_j . (c0, c1) mod q_i),
 *   r_j = t_j if G_j = 1, else hexl_hks_rotate_hoisted(&giant_hks[j], &G_j, 1, ., t_j, l),
 *   d_out = sum_j r_j mod q_i, every word canonical.
 * The call is word for word that composition: both building blocks end in canonical residues of exactly defined classes, so storing the
 * baby products instead of recomputing them per row, and the order of accumulation, cannot change a word. With alpha = 1, K = L + 1 and
 * n_limbs = L it equals hexl_linear_transform_bsgs word for word on per-limb plans keyed from the same device buffers. It is NOT word for
 * word what these routes give, which all decrypt alike: R calls of hexl_hks_rotate weighted and summed by the caller (the lifts of a
 * permuted digit differ, as above), and the flat hexl_hks_linear_transform over the n_baby x n_giant composed rotations (one rounding by
 * P instead of one per row and one per rotated giant step).
 * Noise, under the assumptions of the bound above: sum_j B_lt(row j) + #{j : G_j != 1} . B, with B_lt the linear transform's bound for
 * row j's plaintexts and B the key switch's; sigma_G is a signed permutation and preserves the infinity norm, identity-only rows add nothing.
 * HEXL_E_BADARG: a null argument or array, d_pt_identity excepted (batch == 0 does not excuse it); n_giant == 0; no object at all; a giant
 * row with neither a plaintext nor an identity term; objects that do not share the first one's plan and alpha; a NULL baby object whose
 * column has a plaintext; a NULL giant object with G_j != 1; n_limbs outside 1 ... L; an element that is even or >= 2n, used or not;
 * d_out overlapping d_ct, any plaintext or any identity plaintext; a size or a grid that overflows, including an n_baby for which not
 * one instance fits the baby store. Then HEXL_E_NOKEYS if any object that is USED has no keys (an unused one may lack them). Then
 * batch == 0 returns 0 with nothing written. n_baby == 0 is allowed when every row has its identity term.
 * Asynchronous on the context's stream, on one lane; the host arrays may be reused on return. Precondition: every input word is below
 * its modulus; like the rest of the hybrid family this call does NOT raise the input-range flag (hexl_ks_range_check).
 * Device memory on the scratch owner, grow-only: the hoisted calls' scratch, the baby store (n_baby x chunk x 2 x K x n doubles) and
 * t_j (chunk x 2 x L x n words); chunk is the key switch's, cut so that the baby store stays within 2 GiB (never below one instance)
 * unless HEXL_KS_CHUNK forces it. hexl_hks_bsgs_scratch_bytes(hks, n_baby, batch) is that sum; hexl_hks_scratch_bytes and
 * hexl_hks_hoisted_scratch_bytes are unchanged. */
int hexl_hks_linear_transform_bsgs(hexl_hks* const* baby_hks, const uint64_t* baby_elts, size_t n_baby, hexl_hks* const* giant_hks, const uint64_t* giant_elts, size_t n_giant, const uint64_t* const* d_pts, const uint64_t* const* d_pt_identity, uint64_t* d_out, const uint64_t* d_ct, size_t batch, uint64_t n_limbs);
size_t hexl_hks_bsgs_scratch_bytes(const hexl_hks* hks, size_t n_baby, size_t batch);
/* The double-hoisted BSGS: the same sum with the giant steps kept in the extended basis and ONE division per call --
 * by P, or with rescale = 1 by R = P q_(l-1), which folds the hexl_rescale that ends every linear layer into the same mod-down. Per
 * instance U + #{G != 1} (D/2 + U) + D transforms (U = l + sum_d (l + n_p - |G_d|), D = 2 n_p + 2 l) where hexl_hks_linear_transform_bsgs
 * runs U + n_giant D + #{G != 1} (U + D); the keys are the same n_baby + n_giant.
 * Arguments, layouts and the scratch-owner rule are exactly those of hexl_hks_linear_transform_bsgs: objects on one plan with one alpha,
 * plaintexts [K][n] that serve every level, diagonal (j, i) already rotated by G_j^-1, NULL entries where unused. d_ct is
 * [batch][2][l][n]; d_out is WRITTEN, [batch][2][l][n] for rescale == 0 and [batch][2][l - 1][n] for rescale == 1 (l >= 2).
 * Definition (normative), per instance, every line modulo its limb's modulus, every stored word canonical; rows r run over
 * T_l = {0 .. l-1} + S, sigma_g is the word permutation of hexl_apply_galois, steps 1-4 and 3'-4' are those of hexl_hks_keyswitch and
 * hexl_hks_relinearize_rescale:
 *   1  ext = steps 1-2 applied to c1.
 *   2  for every row j: inner_j[k][r] = sum_i pt_{j,i}[r] (sum_d sigma_{g_i}(ext_d[r]) key_i[d][k][r]) over row j's non-NULL terms (the acc
 *      of hexl_hks_linear_transform; 0 for an identity-only row); kf_j[0][i] = sum_i pt_{j,i}[i] sigma_{g_i}(c0[i]) + pt_id_j[i] c0[i] and
 *      kf_j[1][i] = pt_id_j[i] c1[i] for i < l.
 *   3  A on T_l and F on the data limbs start at 0.
 *      G_j = 1:  A[k] += inner_j[k], F[k] += kf_j[k].
 *      G_j != 1: u_j[i] = kf_j[1][i] + down_P(inner_j[1])[i], canonical, down_P = step 4 on component 1 only (word for word component 1
 *                of hexl_hks_linear_transform(row j)); W_j[k][r] = sum_d sigma_{G_j}(ext'_d[r]) key_{G_j}[d][k][r] with ext' = steps 1-2
 *                applied to u_j; A[0] += sigma_{G_j}(inner_j[0]) + W_j[0] (sigma acts on every row of T_l, the special rows included);
 *                A[1] += W_j[1]; F[0] += sigma_{G_j}(kf_j[0]).
 *   4  rescale == 0: out[k][i] = F[k][i] + down_P(A[k])[i], step 4 with result = F.
 *      rescale == 1: steps 3'-4' with d_k = F[k] and acc = A: X_k = P F_k + A_k modulo Q_l P is divided by R from the sources S + {l - 1}.
 * Every output word is the canonical residue of an exactly defined class: the order of accumulation cannot change a word.
 * Facts: with n_giant = 1, G = 1, rescale = 0 the call is word for word hexl_hks_linear_transform on row 0. A grid whose giant elements are
 * all 1, rescale = 0, is word for word the flat hexl_hks_linear_transform over the concatenated non-NULL terms (objects and elements repeat
 * per row; at most one row carries an identity term). With rescale = 1, per coefficient out_k = round(X_k / R) - e with an integer e in
 * [0, n_p] (the argument of DESIGN.md 4.6.13). With some G_j != 1 the call is NOT word for word hexl_hks_linear_transform_bsgs: component 0
 * of a row is no longer rounded before the giant step; with rescale = 1 it is NOT word for word that call followed by hexl_rescale. All of
 * these decrypt alike.
 * Noise, under the assumptions of the bounds above, with E = 21 n sum_d |G_d| D_d and S_j = sum_i ||pt_{j,i}||_1:
 *   (sum_j S_j E + #{G != 1} (E + P (n_p + 1/2) n)) / P + (n_p + 1/2)(n + 1),  the first term divided by q_(l-1) as well with rescale = 1
 * (then against the exact result divided by q_(l-1)). The term P (n_p + 1/2) n is the rounding of u_j carried through the giant switch.
 * Errors: the checks of hexl_hks_linear_transform_bsgs in its order -- HEXL_E_BADARG, then HEXL_E_NOKEYS for an object that is USED, then
 * batch == 0 -- and HEXL_E_BADARG also for rescale outside {0, 1} and for n_limbs < 2 with rescale == 1; the overlap checks use the
 * output's real size. Asynchronous on the context's stream, on one lane; the host arrays may be reused on return; the call does NOT raise
 * the input-range flag (hexl_ks_range_check).
 * Device memory on the scratch owner, grow-only: what hexl_hks_linear_transform_bsgs holds at the same chunk, A (chunk x 2 x K x n
 * doubles) and, for rescale == 1, F (chunk x 2 x L x n words, the buffer hexl_hks_multiply_sum_rescale keeps its (d0, d1) in).
 * hexl_hks_bsgs_ext_scratch_bytes(hks, n_baby, batch, rescale) is that sum; the four older *_scratch_bytes figures are unchanged. */
int hexl_hks_linear_transform_bsgs_ext(hexl_hks* const* baby_hks, const uint64_t* baby_elts, size_t n_baby, hexl_hks* const* giant_hks, const uint64_t* giant_elts, size_t n_giant, const uint64_t* const* d_pts, const uint64_t* const* d_pt_identity, uint64_t* d_out, const uint64_t* d_ct, size_t batch, uint64_t n_limbs, int rescale);
size_t hexl_hks_bsgs_ext_scratch_bytes(const hexl_hks* hks, size_t n_baby, size_t batch, int rescale);
/* The hybrid multiply: a sum of ciphertext products, its relinearisation on the hybrid key and -- the two rescaling
 * calls -- the rescale, in one call. On the hybrid gadget a product is otherwise hexl_ct_tensor_sum, hexl_hks_relinearize and
 * hexl_rescale: the three-component sum and the un-rescaled ciphertext each pass through memory, and two mod-downs run (by P, then by
 * q_(l-1)): 2 n_p + 4 l transforms per instance behind the multiply-accumulate. The rescaling calls divide ONCE, by R = P q_(l-1) from the
 * source basis S and {l - 1}: 2 n_p + 2 l transforms (L = 12, alpha = 4, n_p = 4: 80 instead of 104) and one rounding instead of two.
 *   d_as, d_bs, in_limbs, n_terms   as for hexl_ct_tensor_sum: HOST arrays of 1 ... 8 DEVICE operands [batch][2][in_limbs][n], in_limbs
 *               NULL or 2 n_terms entries in l ... K; every operand is read through its first l limbs; d_bs[t] may be d_as[t].
 *   n_limbs = l the level of the product. d_ct3 DEVICE [batch][3][l][n] = (d0, d1, d2).
 *   hexl_hks_multiply_sum_relinearize   1 <= l <= L. d_out [batch][2][l][n] WRITTEN, word for word
 *               hexl_ct_tensor_sum(plan, tmp, d_as, d_bs, in_limbs, n_terms, batch, l) then hexl_hks_relinearize(hks, d_out, tmp, batch, l);
 *               the three-component sum never exists in memory.
 *   hexl_hks_relinearize_rescale        2 <= l <= L. d_out [batch][2][l - 1][n] WRITTEN, as defined below.
 *   hexl_hks_multiply_sum_rescale       2 <= l <= L. d_out [batch][2][l - 1][n] WRITTEN, word for word hexl_ct_tensor_sum at level l then
 *               hexl_hks_relinearize_rescale; neither the three-component sum nor an un-rescaled ciphertext exists in memory.
 * hexl_hks_relinearize_rescale per instance, every line modulo its limb's modulus and every stored word canonical (normative):
 *   1-3 steps 1-3 of the hexl_hks_keyswitch definition applied to t = d2 at level l: acc[k][j] for k in {0, 1}, j in T_l
 *   3'  acc'[k][i] = acc[k][i] + (P mod q_i) . d_k[i] for i < l;  acc'[k][s] = acc[k][s] for s in S
 *       (P d_k vanishes modulo every special prime: acc'[k] is the residue vector of X_k = P d_k + KSacc_k modulo Q_l P)
 *   4'  R = P q_(l-1) (odd), h = (R - 1) / 2, B = S and {l - 1}:
 *       for s in B   b_s = INTT_s(acc'[k][s]) + (h mod q_s),  z_s = b_s . ((R / q_s)^-1 mod q_s);
 *       for i < l - 1   w_i = sum_{s in B} z_s . ((R / q_s) mod q_i)  and
 *         out[k][i] = (acc'[k][i] - NTT_i((w_i + fix_i) mod q_i)) . (R^-1 mod q_i),  fix_i = q_i - (h mod q_i)
 * Consequence: for every coefficient out_k = round(X_k / R) - e with e an integer in [0, n_p] -- the uncorrected conversion from the
 * n_p + 1 sources overshoots by at most n_p multiples of R. The fused result is therefore NOT word for word hexl_hks_relinearize
 * followed by hexl_rescale: that route rounds twice, this one once. Both decrypt alike.
 * Noise: for CBD21 key errors and a ternary secret, with D(s) = d0 + d1 s + d2 s^2 lifted centred modulo Q_l, out_0 + out_1 s equals
 * D(s) / q_(l-1) up to an error of infinity norm at most
 *   21 n sum_d |G_d| D_d / (P q_(l-1)) + (n_p + 1/2)(n + 1).
 * All three are asynchronous on the context's stream, on one lane; the host arrays may be reused on return. Precondition: every input
 * word is below its modulus; like the rest of the hybrid family they do NOT raise the input-range flag (hexl_ks_range_check).
 * HEXL_E_BADARG: a null handle, pointer or array entry (batch == 0 does not excuse it); n_terms outside 1 ... 8; n_limbs outside its
 * range (the lower bound is 2 for the two rescaling calls); an in_limbs entry outside l ... K; d_out overlapping any operand or d_ct3; a
 * size or a grid that overflows. Then HEXL_E_NOKEYS before hexl_hks_set_keys_device; then batch == 0 returns 0 with nothing written.
 * Device memory on the object, grow-only, beside the key switch's scratch: the slice buffer of hexl_hks_relinearize (chunk x L x n words:
 * component 2 of one chunk's tensor sums) and, for hexl_hks_multiply_sum_rescale, (d0, d1) of one chunk (chunk x 2 x L x n words).
 * hexl_hks_relinearize_rescale reads d0, d1 and d2 where they lie and needs neither. hexl_hks_mul_scratch_bytes(hks, batch) is
 * hexl_hks_scratch_bytes plus both buffers; hexl_hks_scratch_bytes, hexl_hks_hoisted_scratch_bytes and hexl_hks_bsgs_scratch_bytes are
 * unchanged. */
int hexl_hks_multiply_sum_relinearize(hexl_hks* hks, uint64_t* d_out, const uint64_t* const* d_as, const uint64_t* const* d_bs, const uint64_t* in_limbs, size_t n_terms, size_t batch, uint64_t n_limbs);
int hexl_hks_relinearize_rescale(hexl_hks* hks, uint64_t* d_out, const uint64_t* d_ct3, size_t batch, uint64_t n_limbs);
int hexl_hks_multiply_sum_rescale(hexl_hks* hks, uint64_t* d_out, const uint64_t* const* d_as, const uint64_t* const* d_bs, const uint64_t* in_limbs, size_t n_terms, size_t batch, uint64_t n_limbs);
size_t hexl_hks_mul_scratch_bytes(const hexl_hks* hks, size_t batch);
/* Arithmetic tier per limb (introspection for logs and tests): tiers[i], i < key_modulus_size, = the forward transforms' range-
 * reduction period modulo q_i on the FP64 path -- 12 / 6 / 3 for q_i <= 2^49 / 2^50 / 2^51 (1 + 2^-7), 0 = every value reduced after
 * every operation (q_i up to 2^52); -1 for every limb of a plan on the integer kernels (a modulus >= 2^52). Every transform runs modulo
 * ONE q_i and takes that limb's tier, as each NTT engine of the reference runs on its own modulus (device/keyswitch/ntt_core.hpp:285-291);
 * HEXL_KS_PER_LIMB=0 gives every limb the tier of the plan's largest modulus. Returns 1 when the limbs in use differ in tier, else 0. */
int hexl_ks_plan_tiers(const hexl_ks_plan* plan, int* tiers /* [key_modulus_size] */);
/* bytes of HBM scratch a batch of `batch` keyswitches needs (for capacity planning) */
size_t hexl_ks_scratch_bytes(const hexl_ks_plan* plan, size_t batch);

/* Host-pointer entry points used by the C++ API layer (libhexl-fpga.so): pinned staging + H2D/D2H
 * around the launchers above; synchronous on return. Every object is passed by its own pointer -- the
 * reference needs batch elements contiguous for NTT/INTT/dyadic (one memcpy from the first object,
 * host/src/fpga.cpp:379-388,405-406) and copies keyswitch objects one by one (fpga.cpp:542-555); per-object
 * pointers are a superset of both. */
int hexl_ntt_fwd_host(hexl_ctx* ctx, uint64_t* const* h_x, size_t batch, const uint64_t* h_roots,
                      const uint64_t* h_precon, uint64_t q, uint64_t n);
int hexl_ntt_inv_host(hexl_ctx* ctx, uint64_t* const* h_x, size_t batch, const uint64_t* h_inv_roots,
                      const uint64_t* h_inv_precon, uint64_t q, uint64_t inv_n,
                      uint64_t inv_n_w, uint64_t n);
int hexl_dyadic_multiply_host(hexl_ctx* ctx, uint64_t* const* h_out, const uint64_t* const* h_a,
                              const uint64_t* const* h_b, size_t batch, uint64_t n,
                              const uint64_t* const* h_moduli, uint64_t n_moduli);
int hexl_keyswitch_host(hexl_ks_plan* plan, uint64_t* const* h_results,
                        const uint64_t* const* h_t_targets, size_t batch);

/* timing hook for bench.py: average milliseconds per keyswitch launch and per stage (s1: steps 1-2, inverse
 * transforms + mod-up transforms; s2: steps 3-4, multiply-accumulate + special-prime inverse; s3: steps 5-7,
 * mod-down) over `iters` launches of a batch that fits one scratch chunk, measured with hipEvents on the
 * context's stream. */
int hexl_ks_time_stages(hexl_ks_plan* plan, uint64_t* d_result, const uint64_t* d_t_target,
                        size_t batch, int iters, float* ms_out /* [4]: total, s1, s2, s3 */);

#ifdef __cplusplus
}
#endif
#endif /* HEXL_MI355X_H */
