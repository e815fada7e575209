// The 4-simplex walk over a LUT that lives in LDS, defined once: the tile-fused kernels (lerf_fused_impl.h: byte LUTs of
// stage 1 and LeRF-L, packed dword pieces of LeRF-G), the LDS-resident LUT pass (lerf_lut_interp.hip) and the
// micro-benchmarks (tools/ubench) all compile these functions.  gfx950 only; nothing here depends on a tile shape, a
// channel count or a workgroup size.  (The portable global-memory walk of the direct kernels is simplex_path in
// lerf_common.h; the training kernels have a walk of their own with another tie rule.)
#pragma once

#include "lerf_common.h"

namespace lerf {

// ---------------------------------------------------------------------------
// simplex walk (index/weight computation only).  Keys are (LSB << 16) | axis stride so that one unsigned sort orders
// the four axes by decreasing LSB (ties: zero weight, any order).  STRIDE_SCALE = bytes per LUT entry, folded into
// the strides so the indices are byte offsets.
//
// Instruction budget (gfx950 issues v_and/or/add/sub/lshr in ~2.4 cycles per wave64, every 3-operand or min/max/
// shift-left/24-bit-multiply op in ~4.3: profiles/r01_valu_instruction_rates.txt), per lookup:
//   keys      3 x (v_and + v_lshl_or)                       the centre key is shared by the rotations of a position
//   sort      7 three-input ops  m = max3(a,b,c)  e = med3(a,b,c)  n = min3(a,b,c)
//                                s0 = max(m,d)  s1 = med3(m,e,d)  s2 = med3(e,n,d)  s3 = min(n,d)
//             instead of the 10 of a 5-comparator network
//   indices   the walk ends at base + (all four strides), a constant: vertex 4 is an immediate offset on vertex 0 and
//             vertex 3 = vertex 4 - stride(s3), so only s0, s1, s3 contribute an AND + ADD/SUB (s2 is needed for its
//             LSB alone)
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned umax3(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_max3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ unsigned umed3(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ unsigned umin3(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// LDS accesses by 32-bit LDS address.  A dynamic LDS array is a link-time symbol: pointer arithmetic on it leaves one
// "+ smem" per distinct address chain in the instruction stream (v_add 0); folding the table's LDS address into the walk's
// base index once per position removes them, and constant parts still fold into the DS immediate offset.
typedef __attribute__((address_space(3))) const uint32_t lds_cu32_t;
typedef __attribute__((address_space(3))) const int8_t lds_ci8_t;
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}
// OFF is applied as a constant element index so that it lands in the DS immediate offset
template <int OFF = 0>
__device__ __forceinline__ uint32_t lds_ld32(uint32_t a) { return ((lds_cu32_t*)a)[OFF / 4]; }
template <int OFF = 0>
__device__ __forceinline__ int lds_ldi8(uint32_t a) { return (int)((lds_ci8_t*)a)[OFF]; }

// A tile pixel is needed twice: its LSB in bits 16..19 of the sort key and its MSB as an index digit.  ds_read_u8_d16_hi
// returns the byte in bits 16..23 (v << 16 for free; what it leaves in the low half is not relied upon), so that
//   key = (r & 0x000F0000) | stride   one v_and_or_b32          msb = r >> 20   one v_lshrrev_b32
// instead of v_and + v_lshl_or + v_lshrrev on a zero-extended byte.  The compiler does not track inline-asm LDS
// loads: the caller waits for them with an s_waitcnt that names the registers, so that every use is ordered behind it.
__device__ __forceinline__ uint32_t lds_pixel_hi(uint32_t addr) {
    uint32_t r;
    asm volatile("ds_read_u8_d16_hi %0, %1" : "=v"(r) : "v"(addr));
    return r;
}
template <int OFF>
__device__ __forceinline__ uint32_t lds_pixel_hi_off(uint32_t addr) {
    uint32_t r;
    asm volatile("ds_read_u8_d16_hi %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
    return r;
}
__device__ __forceinline__ unsigned key_of(uint32_t r, unsigned stride) {
    unsigned k;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(k) : "v"(r), "s"(0x000F0000u), "v"(stride));
    return k;
}
__device__ __forceinline__ unsigned msb_of(uint32_t r) { return r >> 20; }

// acc + d.lo16 * key.hi16 (signed): one Abel term of a byte-LUT walk, the LSB taken from the sorted key's high half in place --
// sub + mad per term instead of sub + multiply (SDWA) + half a three-input add (-2 of ~30 instructions per walk; the
// 24-bit multiply on the extracted LSB was the form it replaced)
__device__ __forceinline__ int mad_i16_keyhi(int d, unsigned key, int acc) {
    asm("v_mad_i32_i16 %0, %1, %2, %0 op_sel:[0,1,0,0]" : "+v"(acc) : "v"(d), "v"(key));
    return acc;
}

// acc + w.lo24 * d.lo24 in one instruction.  Written out because the compiler does not always form it: behind a function
// boundary it pairs the products of a slot into v_mul_u32_u24 x 2 + v_add3_u32 instead (+5 instructions per stage-2 slot).
__device__ __forceinline__ uint32_t mad_u24(uint32_t w, uint32_t d, uint32_t acc) {
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(w), "v"(d), "v"(acc));
    return r;
}

// acc + w.lo16 * d.hi16: the upper half of a packed stage-2 entry multiplied in place (op_sel picks the high half of src1)
__device__ __forceinline__ uint32_t mad_hi16(uint32_t w, uint32_t d, uint32_t acc) {
    asm("v_mad_u32_u16 %0, %1, %2, %0 op_sel:[0,1,0,0]" : "+v"(acc) : "v"(w), "v"(d));
    return acc;
}

template <int STRIDE_SCALE>
struct Walk {
    static constexpr int ALL = (kStrideA + kStrideB + kStrideC + kStrideD) * STRIDE_SCALE;   // vertex 4 - vertex 0
    int i0, i1, i2, i3m;        // byte offsets of vertices 0, 1, 2 and (vertex 3 - ALL); vertex 4 = i0 + ALL
    unsigned f0, f1, f2, f3;    // sorted LSBs
    unsigned k0, k1, k2, k3;    // the sorted keys themselves (LSB in the high half: a v_mad_*_i16 reads it there with op_sel)
    // vertex n = address a(n) + constant c(n): the constant goes into the DS immediate offset
    __device__ __forceinline__ uint32_t a(int n) const { return (uint32_t)(n == 0 ? i0 : n == 1 ? i1 : n == 2 ? i2 : n == 3 ? i3m : i0); }
    static constexpr int c(int n) { return n >= 3 ? ALL : 0; }
    __device__ __forceinline__ uint32_t ld32(int n) const { return n >= 3 ? lds_ld32<ALL>(a(n)) : lds_ld32<0>(a(n)); }
    __device__ __forceinline__ int ldi8(int n) const { return n >= 3 ? lds_ldi8<ALL>(a(n)) : lds_ldi8<0>(a(n)); }
};

// ka = key of the centre pixel, basea = its MSB contribution to the index (both shared by the rotations of a position);
// rb, rc, rd = the other three pixels as lds_pixel_hi() returned them; sb, sc, sd = the axis strides (bytes) in VGPRs
template <int STRIDE_SCALE>
__device__ __forceinline__ Walk<STRIDE_SCALE> simplex_walk(unsigned ka, int basea, uint32_t rb, uint32_t rc, uint32_t rd,
                                                           unsigned sb, unsigned sc, unsigned sd) {
    Walk<STRIDE_SCALE> W;
    const unsigned kb = key_of(rb, sb), kc = key_of(rc, sc), kd = key_of(rd, sd);
    // base index, Horner over the MSBs: ((b * 17 + c) * 17 + d) * scale + a-part
    const unsigned t = __umul24(__umul24(msb_of(rb), (unsigned)kL) + msb_of(rc), (unsigned)kL) + msb_of(rd);
    W.i0 = basea + (int)(t * STRIDE_SCALE);
    const unsigned m = umax3(ka, kb, kc), e = umed3(ka, kb, kc), n = umin3(ka, kb, kc);
    const unsigned s0 = m > kd ? m : kd;
    const unsigned s1 = umed3(m, e, kd);
    const unsigned s2 = umed3(e, n, kd);
    const unsigned s3 = n < kd ? n : kd;
    W.i1 = W.i0 + (int)(s0 & 0xFFFFu);
    W.i2 = W.i1 + (int)(s1 & 0xFFFFu);
    W.i3m = W.i0 - (int)(s3 & 0xFFFFu);
    W.f0 = s0 >> 16; W.f1 = s1 >> 16; W.f2 = s2 >> 16; W.f3 = s3 >> 16;
    W.k0 = s0; W.k1 = s1; W.k2 = s2; W.k3 = s3;
    return W;
}

// One walk of a byte LUT from its four pixels (ra = the centre: the slowest axis); lut_a = LDS address of the LUT
__device__ __forceinline__ Walk<1> simplex_walk_px(uint32_t lut_a, uint32_t ra, uint32_t rb, uint32_t rc, uint32_t rd) {
    const unsigned ka = key_of(ra, kStrideA);
    // LDS address of the base corner, as one multiply-add on the stride register the key already uses (4913 is no inline
    // constant: left to the compiler it becomes a multiply by a literal and an add, +1 instruction per walk)
    const int basea = (int)mad_u24(msb_of(ra), kStrideA, lut_a);
    return simplex_walk<1>(ka, basea, rb, rc, rd, kStrideB, kStrideC, kStrideD);
}

// byte LUTs: the five corners of a walk, and what they contribute to the numerator
//   sum_n w_n P_n = 16 P_0 + sum_n f_n (P_{n+1} - P_n)   (w_0 = 16 - f_0, w_n = f_{n-1} - f_n, w_4 = f_3):
// four multiply-adds and four subtractions per lookup instead of five weights + five multiply-adds.  byte_abel() adds the
// f_n terms to acc; the caller supplies 16 P_0 (as the start value, or summed over the walks of a position).
struct ByteCorners { int e0, e1, e2, e3, e4; };
__device__ __forceinline__ ByteCorners byte_gather(const Walk<1>& W) {
    ByteCorners E;
    E.e0 = W.ldi8(0); E.e1 = W.ldi8(1); E.e2 = W.ldi8(2); E.e3 = W.ldi8(3); E.e4 = W.ldi8(4);
    return E;
}
__device__ __forceinline__ int byte_abel(const Walk<1>& W, const ByteCorners& E, int acc) {
    acc = mad_i16_keyhi(E.e1 - E.e0, W.k0, acc);
    acc = mad_i16_keyhi(E.e2 - E.e1, W.k1, acc);
    acc = mad_i16_keyhi(E.e3 - E.e2, W.k2, acc);
    acc = mad_i16_keyhi(E.e4 - E.e3, W.k3, acc);
    return acc;
}

}  // namespace lerf
