// ls_device.h -- the one home of the device-side leaf helpers (gfx950, wave64): vector types, the two-piece f16 split and its per-row
// power-of-two scale, the DPP lane reductions, the VN activation and the four-channel xyz triple.  Kernels that must agree bit for bit
// (table path / fused destination side / table-free layers, the GEMM family, the k-NN filter's image) take this arithmetic from here.
// Merge rule: two helpers are one only when their bodies are the same operations in the same order; where they are not, they stay apart
// and say why (amax4 / amax_f4 below; block_sum_256 in pointwise.hip, block_sum_256_opt in optim.hip, block_sum_1024 in icp.hip).
#pragma once
#include "ls_common.h"

namespace ls {

typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

// XCD-aware block remap (MI355X: block b is dispatched to XCD b % 8, each XCD has a private 4 MiB L2).
// Returns a logical block id such that the blocks resident on one XCD cover a CONTIGUOUS range of logical
// ids, so consecutive logical ids (tiles of the same instance) share an L2.  Bijective for any nblocks.
__device__ __forceinline__ int xcd_remap(int bid, int nblocks) {
    const int q = nblocks / kXcds, r = nblocks % kXcds;
    const int xcd = bid % kXcds, slot = bid / kXcds;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + slot;
}

// ---------------------------------------------------------------------------------------------- lane reductions
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// reductions inside aligned groups of 16 lanes (one attention head = 16 channels = one DPP row)
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// LS_DPP_NOP=n (dev builds only, scripts/diag/pk_hazard_repro.sh): n + 1 wait states between the instruction that produces a DPP operand and the DPP
// instruction that reads it from other lanes -- the s_nop sweep of the reproducibility defect described at edge_attn_v4_kernel
#ifdef LS_DPP_NOP
#define LS_DPP_STR2(x) #x
#define LS_DPP_STR(x) LS_DPP_STR2(x)
#define LS_DPP_FENCE(v) asm volatile("s_nop " LS_DPP_STR(LS_DPP_NOP) : "+v"(v))
#else
#define LS_DPP_FENCE(v)
#endif
// one DPP step of a float reduction: v (+ | max) the value the control word CTRL brings from another lane
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    LS_DPP_FENCE(v);
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL, int ROWMASK = 0xF>
__device__ __forceinline__ float dpp_max(float v) {
    LS_DPP_FENCE(v);
    return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROWMASK, 0xF, false)));
}
__device__ __forceinline__ float quad_sum(float v) { return dpp_add<0x4E>(dpp_add<0xB1>(v)); }
__device__ __forceinline__ float quad_max(float v) { return dpp_max<0x4E>(dpp_max<0xB1>(v)); }
template <int LPP>
__device__ __forceinline__ float group_sum(float v) {  // all-reduce over aligned groups of LPP lanes
    v = quad_sum(v);
    v = dpp_add<0x141>(v);  // row_half_mirror
    v = dpp_add<0x140>(v);  // row_mirror -> 16-lane sum in every lane
    if constexpr (LPP >= 32) v += __shfl_xor(v, 16, 64);
    if constexpr (LPP >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}
template <int LPP>
__device__ __forceinline__ float group_max(float v) {  // all-reduce (max) over aligned groups of LPP lanes
    v = dpp_max<0x140>(dpp_max<0x141>(dpp_max<0x4E>(dpp_max<0xB1>(v))));
    if constexpr (LPP >= 32) v = fmaxf(v, __shfl_xor(v, 16, 64));
    if constexpr (LPP >= 64) v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}
// max over aligned groups of 8 lanes (the 8 staging threads of one operand row) / 16 lanes, in every lane of the group
__device__ __forceinline__ float max8(float v) { return dpp_max<0x141>(dpp_max<0x4E>(dpp_max<0xB1>(v))); }
__device__ __forceinline__ float max16(float v) { return dpp_max<0x140>(max8(v)); }
// wave maximum on the DPP network (no LDS crossbar): the result is valid in LANE 63 only
__device__ __forceinline__ float wave_max_lane63(float v) {
    v = dpp_max<0xB1>(v);         // quad_perm [1,0,3,2]
    v = dpp_max<0x4E>(v);         // quad_perm [2,3,0,1]
    v = dpp_max<0x141>(v);        // row_half_mirror
    v = dpp_max<0x140>(v);        // row_mirror
    v = dpp_max<0x142, 0xA>(v);   // row_bcast15 -> rows 1, 3
    v = dpp_max<0x143, 0xC>(v);   // row_bcast31 -> rows 2, 3
    return v;
}

// max|v| of four values.  The two forms associate differently -- amax4 folds the running maximum m in with the first pair, amax_f4 has none --
// so fmaxf(m, amax_f4(v)) is a different instruction sequence from amax4(m, v): neither is written through the other.
__device__ __forceinline__ float amax4(float m, const float4& v) {
    return fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}
__device__ __forceinline__ float amax_f4(const float4& v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }

// m[r] = max(0, max_q rm[row[r] * parts + q]), r < NR: the parts of NR rows' maxima (GemmAux::a_rowmax) folded, the loads of ALL rows requested before
// the first is used (the loop `for q: m = fmaxf(m, rp[q])` per row compiles to one load and one full wait per part and row: 64 dependent round trips in
// front of a tile at parts = 16).  A trip covers sixteen parts of every row as four 16-byte loads where the rows' parts are 16-byte aligned (parts % 4 == 0
// and an aligned array), eight parts as dwords otherwise; the part index is CLAMPED to the row's last part, not predicated -- max does not mind a repeated
// value, nothing past row * parts + parts - 1 is read, and the trip stays one basic block (gemm_vn_direct_kernel, csv: a conditional load is a branch with
// its own wait).  The encoder's parts (1, 2, 4, 8, 16) are one trip; a larger run-time `parts` (ls_gemm_ex) loops with one wait per trip.  The maximum is
// exact in any order, and fmaxf drops a NaN on either side, as the sequential loop did.
template <int NR>
__device__ __forceinline__ void rowmax_fold(const float* __restrict__ rm, const size_t (&row)[NR], int parts, float (&m)[NR]) {
#pragma unroll
    for (int r = 0; r < NR; ++r) m[r] = 0.f;
    if (parts == 1) {
        float v[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) v[r] = rm[row[r]];
#pragma unroll
        for (int r = 0; r < NR; ++r) m[r] = fmaxf(m[r], v[r]);
    } else if ((parts & 3) == 0 && (reinterpret_cast<uintptr_t>(rm) & 15) == 0) {
        const int p4 = parts >> 2;
        for (int q = 0; q < p4; q += 4) {
            float4 v[NR][4];
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[r][j] = reinterpret_cast<const float4*>(rm + row[r] * parts)[min(q + j, p4 - 1)];
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) m[r] = fmaxf(m[r], fmaxf(fmaxf(v[r][j].x, v[r][j].y), fmaxf(v[r][j].z, v[r][j].w)));
        }
    } else {
        for (int q = 0; q < parts; q += 8) {
            float v[NR][8];
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int j = 0; j < 8; ++j) v[r][j] = rm[row[r] * parts + min(q + j, parts - 1)];
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int j = 0; j < 8; ++j) m[r] = fmaxf(m[r], v[r][j]);
        }
    }
}

// ---------------------------------------------------------------------------------------------- the two-piece f16 split
// a = h + l with h = f16(a) (11 significant bits) and l = f16(a - h) (the residual is exact in fp32 and keeps 11 more bits while it is a
// normal f16): |a - (h + l)| <= 2^-22 |a|.  What the kernels do with the pieces (three MFMAs per 16 k, their order): gemm.hip, "2 x f16 split".
__device__ __forceinline__ void split2_f16_pair(f32x2_t v, unsigned& h, unsigned& l) {
    const f16x2_t hv = __builtin_convertvector(v, f16x2_t);
    const f16x2_t lv = __builtin_convertvector(v - __builtin_convertvector(hv, f32x2_t), f16x2_t);
    h = __builtin_bit_cast(unsigned, hv);
    l = __builtin_bit_cast(unsigned, lv);
}
__device__ __forceinline__ void split2_f16(const float4& v, uint2& h, uint2& l) {
    split2_f16_pair(f32x2_t{v.x, v.y}, h.x, l.x);
    split2_f16_pair(f32x2_t{v.z, v.w}, h.y, l.y);
}
// split of s * v (s: the row's power of two); the multiply is spelled as packed fp32 (v_pk_mul_f32: the file is built without SLP vectorisation)
__device__ __forceinline__ void split2_f16s(const float4& v, float s, uint2& h, uint2& l) {
    const f32x2_t sv = {s, s};
    split2_f16_pair(f32x2_t{v.x, v.y} * sv, h.x, l.x);
    split2_f16_pair(f32x2_t{v.z, v.w} * sv, h.y, l.y);
}
// eight consecutive-k fp32 values -> the (hi, lo) MFMA operand fragments of this lane
__device__ __forceinline__ void split8_f16(const float* p, f16x8_t& h, f16x8_t& l) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    uint4 hh, ll;
    split2_f16_pair(f32x2_t{a.x, a.y}, hh.x, ll.x); split2_f16_pair(f32x2_t{a.z, a.w}, hh.y, ll.y);
    split2_f16_pair(f32x2_t{b.x, b.y}, hh.z, ll.z); split2_f16_pair(f32x2_t{b.z, b.w}, hh.w, ll.w);
    h = __builtin_bit_cast(f16x8_t, hh);
    l = __builtin_bit_cast(f16x8_t, ll);
}
// the same of s * (a | b), values in registers, as the uint4 pair an operand image stores; each pair is scaled where it is split (scalar multiplies: the
// products of split2_f16s's packed one).  Kept beside split8_f16, not merged with it: edge_presplit_wq_kernel scales into an array first and hands on
// f16x8_t fragments, and either change (scaling inside, uint4 results) reorders instructions of that kernel.
__device__ __forceinline__ void split8_f16s(const float4& a, const float4& b, float s, uint4& h, uint4& l) {
    split2_f16_pair(f32x2_t{a.x * s, a.y * s}, h.x, l.x); split2_f16_pair(f32x2_t{a.z * s, a.w * s}, h.y, l.y);
    split2_f16_pair(f32x2_t{b.x * s, b.y * s}, h.z, l.z); split2_f16_pair(f32x2_t{b.z * s, b.w * s}, h.w, l.w);
}

// ---- operand range of the f16 split.  f16 covers 2^-14 .. 65504, fp32 features and gradients do not stay there (a trained encoder's
// conv_c outputs sit at ~1.5e-5 because the heads multiply by scale_factor = 64000, vec_dgcnn_atten.py:234-250; the gradients of the
// pose refinement at 1e-6 .. 1e-8).  So every ROW of A and every row of W is multiplied by its own exact power of two before the split --
// s = 2^(14 - floor(log2 max|row|)): the row's largest element lands in [2^14, 2^15), elements down to 2^-17 of it keep the full 22
// bits (their residual is still a normal f16), below that the absolute error is at most 2^-39 of the row maximum -- 2^-15 of the
// fp32 rounding of the row's largest term -- and the product of the two inverse scales multiplies the fp32 accumulators in
// the epilogue.  Powers of two commute with every rounding in between, so for data that was in range before the result is
// BIT-IDENTICAL to the unscaled split, any finite fp32 input is handled, and a row's result depends on that row's data only.
// The row maxima come from (a) a pre-pass of the kernel over its own operand rows (default), or (b) caller-supplied arrays
// (GemmAux: the decoder chains them from the previous layer's epilogue, weights carry theirs from ls_model_create), which may be
// any upper bound: each factor of two of slack costs one bit at the bottom of the 17-binade window.
// (struct GemmAux: ls_common.h)
// exact powers of two: s * amax in [2^14, 2^15), inv = 1 / s.  amax = 0 (or fp32-subnormal) -> s = 2^126; Inf / NaN rows stay non-finite.
// pow2_scale_be returns the clamped biased exponent of amax; 1 / s follows from it as a float (pow2_inv) or as its exponent (pow2_inv_e = pow2_e of it).
__device__ __forceinline__ unsigned pow2_scale_be(float amax, float& s) {
    unsigned be = (__float_as_uint(amax) >> 23) & 0xffu;
    be = be < 15u ? 15u : be;
    s = __uint_as_float((268u - be) << 23);
    return be;
}
__device__ __forceinline__ float pow2_inv(unsigned be) { return __uint_as_float((be - 14u) << 23); }
__device__ __forceinline__ int pow2_inv_e(unsigned be) { return (int)be - 14 - 127; }
__device__ __forceinline__ void pow2_scale(float amax, float& s, float& inv) { inv = pow2_inv(pow2_scale_be(amax, s)); }
__device__ __forceinline__ void pow2_scale_e(float amax, float& s, int& e_inv) { e_inv = pow2_inv_e(pow2_scale_be(amax, s)); }
// The epilogue's acc * s_a^-1 * s_w^-1: both inverse scales are exact NORMAL powers of two (pow2_scale), so their exponents are kept as
// integers (pow2_e), added, and applied by ONE v_ldexp_f32 -- exact wherever fp32 holds the result, rounded once into the subnormals, never
// an intermediate overflow.  (Until round 4 the two floats were multiplied first: that product flushes to 0 below 2^-149 -- two operand rows
// at ~1e-19 each -- although acc times it can be a normal number.)  In range the result is bit-identical to the multiply.
__device__ __forceinline__ int pow2_e(float p) { return (__float_as_int(p) >> 23) - 127; }
__device__ __forceinline__ float scale_pow2(float acc, int e) { return __builtin_ldexpf(acc, e); }

// ---------------------------------------------------------------------------------------------- VN arithmetic
// canonical squared-difference accumulation (oracle/ls_oracle.c acc_sq)
template <bool FMA>
__device__ __forceinline__ float acc_sq(float d, float diff) {
    if constexpr (FMA) return __fmaf_rn(diff, diff, d);
    else return __fadd_rn(d, __fmul_rn(diff, diff));
}

// VN activation closed form (vec_layers.py:241-268): y - (1-slope) * min(<y,k^>,0) * k^,  k^ = k / max(|k|,1e-12).
// With p = <y,k> un-normalised this is  y - (1-slope) * min(p,0) / max(|k|^2, 1e-24) * k : one v_rcp_f32 instead of a
// correctly rounded sqrt and division (~14 instead of ~40 VALU operations per 3-vector; the edge kernels apply it per edge and
// channel).  Differs from the reference's operation order at the 1e-7 level, like the rest of the folded edge-conv.
// Every multiply-add is SPELLED as an fma (round 3): with -ffp-contract=fast the compiler chose which products to fuse per call site, and
// two kernels that must agree bit for bit (the fused-destination attention kernel and the table path) stopped agreeing in the last bit
// once their loops were restructured differently.
__device__ __forceinline__ void vn_act(float& y0, float& y1, float& y2, float k0, float k1, float k2, float one_minus_slope) {
    const float n2 = __builtin_fmaf(k2, k2, __builtin_fmaf(k1, k1, k0 * k0));
    const float p = __builtin_fmaf(y2, k2, __builtin_fmaf(y1, k1, y0 * k0));
    const float f = one_minus_slope * fminf(p, 0.0f) * __builtin_amdgcn_rcpf(fmaxf(n2, 1e-24f));
    y0 = __builtin_fmaf(-f, k0, y0); y1 = __builtin_fmaf(-f, k1, y1); y2 = __builtin_fmaf(-f, k2, y2);
}

// 1 / max(sqrt(ss), 1e-12) (channel_equi_vec_normalize's Frobenius norm, vec_layers.py:24-31) as ONE v_rsq_f32 on the clamped square
// instead of a correctly rounded sqrt + IEEE division (~18 issue slots per neighbour in the K branch); 1 ulp, far inside the tolerance
__device__ __forceinline__ float inv_fro(float ss) { return __builtin_amdgcn_rsqf(fmaxf(ss, 1e-24f)); }

struct F43 { float4 x, y, z; };  // one xyz triple for four channels
__device__ __forceinline__ F43 ld43(const float* p, int stride) {   // p: global (table row, stride = ldt) or LDS (slab row)
    F43 r;
    r.x = *reinterpret_cast<const float4*>(p);
    r.y = *reinterpret_cast<const float4*>(p + stride);
    r.z = *reinterpret_cast<const float4*>(p + 2 * stride);
    return r;
}
__device__ __forceinline__ F43 add43(const F43& a, const F43& b) {
    F43 r;
    r.x = make_float4(a.x.x + b.x.x, a.x.y + b.x.y, a.x.z + b.x.z, a.x.w + b.x.w);
    r.y = make_float4(a.y.x + b.y.x, a.y.y + b.y.y, a.y.z + b.y.z, a.y.w + b.y.w);
    r.z = make_float4(a.z.x + b.z.x, a.z.y + b.z.y, a.z.z + b.z.z, a.z.w + b.z.w);
    return r;
}
// VN activation on four channels in place (y := act(y, k))
__device__ __forceinline__ void act43(F43& y, const F43& k, float oms) {
    vn_act(y.x.x, y.y.x, y.z.x, k.x.x, k.y.x, k.z.x, oms);
    vn_act(y.x.y, y.y.y, y.z.y, k.x.y, k.y.y, k.z.y, oms);
    vn_act(y.x.z, y.y.z, y.z.z, k.x.z, k.y.z, k.z.z, oms);
    vn_act(y.x.w, y.y.w, y.z.w, k.x.w, k.y.w, k.z.w, oms);
}
// (explicit fma chain, in this order: see vn_act)
__device__ __forceinline__ float dot43(const F43& a, const F43& b) {
    float s = a.x.x * b.x.x;
    s = __builtin_fmaf(a.y.x, b.y.x, s); s = __builtin_fmaf(a.z.x, b.z.x, s);
    s = __builtin_fmaf(a.x.y, b.x.y, s); s = __builtin_fmaf(a.y.y, b.y.y, s); s = __builtin_fmaf(a.z.y, b.z.y, s);
    s = __builtin_fmaf(a.x.z, b.x.z, s); s = __builtin_fmaf(a.y.z, b.y.z, s); s = __builtin_fmaf(a.z.z, b.z.z, s);
    s = __builtin_fmaf(a.x.w, b.x.w, s); s = __builtin_fmaf(a.y.w, b.y.w, s); s = __builtin_fmaf(a.z.w, b.z.w, s);
    return s;
}
// acc += w * y on an xyz triple of four channels
__device__ __forceinline__ void fma43(F43& acc, float w, const F43& y) {
    acc.x.x = __builtin_fmaf(w, y.x.x, acc.x.x); acc.x.y = __builtin_fmaf(w, y.x.y, acc.x.y); acc.x.z = __builtin_fmaf(w, y.x.z, acc.x.z); acc.x.w = __builtin_fmaf(w, y.x.w, acc.x.w);
    acc.y.x = __builtin_fmaf(w, y.y.x, acc.y.x); acc.y.y = __builtin_fmaf(w, y.y.y, acc.y.y); acc.y.z = __builtin_fmaf(w, y.y.z, acc.y.z); acc.y.w = __builtin_fmaf(w, y.y.w, acc.y.w);
    acc.z.x = __builtin_fmaf(w, y.z.x, acc.z.x); acc.z.y = __builtin_fmaf(w, y.z.y, acc.z.y); acc.z.z = __builtin_fmaf(w, y.z.z, acc.z.z); acc.z.w = __builtin_fmaf(w, y.z.w, acc.z.w);
}

}  // namespace ls
