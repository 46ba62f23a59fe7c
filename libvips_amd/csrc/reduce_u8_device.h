// What the uchar reduce kernels on the matrix cores share (reduce_fused_u8.hip, reduce_fused_exch.hip,
// reduce_fused_u8x3.hip, reducev_u8.hip): the operand types, the A-operand tables and the pure helpers that
// turn bytes into B operands and accumulators into bytes.
//
// Every tap runs on the MFMA pipe with v_mfma_f32_4x4x4_16b_f16 (16 independent 4x4x4 blocks, block = 4 lanes):
//
//   B[k][j]  lane j of the block supplies 4 halves = ITS OWN column's bytes of input rows
//            k = 0..3 (a quad of the 8-row group) -- lanes keep their columns, no shuffles
//   A[i][k]  lane i of the block supplies the coefficients of accumulator row i for
//            those 4 rows (the same in all 16 blocks)
//   D[i][j]  lane j, register i: 4 of the 8 live output rows of lane j's column
//
// so one instruction does 16 multiply-adds per lane (v_dot2: 2) on a pipe that the rest of
// the kernel leaves idle.  Exactness: a pixel byte p is used as the f16 DENORMAL with bit
// pattern 0x00pp = p * 2^-24 (one v_perm, no conversion; the MFMA honours f16 denormals,
// tools/mfma_probe.hip), coefficients (|c| < 2048) are exact halves, products are exact in
// f32 and every partial sum is (an integer below 2^23) * 2^-24, so the f32 accumulator holds
// exactly n * 2^-24 with n = sum c * p.  Retire: y = fma(acc, 2^12, 2^-13) = n / 4096 + 2^-13
// exactly, and v_cvt_pk_u8_f32 (round to nearest, saturate 0..255; the 2^-13 turns every
// tie into "up") gives clip((n + 2048) >> 12) -- reduceh.cpp:120-141's rounding -- and
// packs the byte, two instructions per sample.  The host checks the bounds (mfma_taps,
// reduce_u8_host.h).
//
// 8 accumulator rows ("slots") per column rotate through the D <= 8 tap groups: at group g
// (ROT = g mod 8) slot s is d = (ROT - s) mod 8 groups old (d >= D: idle, zero coefficients).
// ROT is a template argument; the A operands come from a 1 KB LDS table indexed by it.
#pragma once

#include "gcn.h"
#include "kernel_stmt.h"
#include "resample.h"

namespace vh {

// (sum + 2048) >> 12, clipped to 0..255 (templates.h:152-157).
//
// The empty asm keeps the shift and the clamp apart on purpose: when hipcc
// (ROCm 7.2) sees shift+clamp of two values being packed into bytes it selects
// gfx950's v_ashr_pk_u8_i32 and then treats bits 31:16 of the result as zero,
// but the hardware leaves the old register contents there -- OR-ing a third
// channel in at bit 16 picked up garbage (found as +1..+9 errors in the blue
// channel only, see DESIGN.md "toolchain findings").
static __device__ __forceinline__ int fin_u8(int s)
{
	s = (s + (INTERPOLATE_SCALE >> 1)) >> INTERPOLATE_SHIFT;
	VH_VECTOR1(s);
	return min(max(s, 0), 255);
}

typedef _Float16 half4v __attribute__((ext_vector_type(4)));
typedef float float4v __attribute__((ext_vector_type(4)));

constexpr int FUSED_THREADS = 256;
constexpr int MFMA_SLOTS = 8;
constexpr int F3_BANDS = 3; // the interleaved-band kernels' band count (reduce_fused_u8x3.hip)

struct MfmaTables {
	// [flip][ROT 8][quad 2][half 2][row 4] x 4 halves
	unsigned short a[2][MFMA_SLOTS * 2 * 2 * 4 * 4];
	unsigned short ah[MFMA_SLOTS * 2 * 2 * 4 * 4]; // the same for the horizontal taps
};

constexpr int MFMA_TABLE_ENTRIES = MFMA_SLOTS * 2 * 2 * 4; // half4v entries per table
constexpr int HSEG_OUT = 8;                                // outputs per horizontal segment

// channel C of rows r0..r3 as four f16 denormals
template <int C>
static __device__ __forceinline__ half4v make_b(unsigned int r0, unsigned int r1, unsigned int r2,
	unsigned int r3)
{
	constexpr unsigned int sel = 0x0c000c00u | (unsigned) C | ((4u + C) << 16);
	uint2 v;
	v.x = __builtin_amdgcn_perm(r1, r0, sel);
	v.y = __builtin_amdgcn_perm(r3, r2, sel);
	return __builtin_bit_cast(half4v, v);
}

// four consecutive T bytes as four f16 denormals
static __device__ __forceinline__ half4v bytes_b(unsigned int w)
{
	uint2 v;
	v.x = __builtin_amdgcn_perm(0u, w, 0x0c010c00u);
	v.y = __builtin_amdgcn_perm(0u, w, 0x0c030c02u);
	return __builtin_bit_cast(half4v, v);
}

// acc = n * 2^-24 -> clip((n + 2048) >> 12) into byte `byte` of `old`
static __device__ __forceinline__ unsigned int fin_pack(float acc, unsigned int byte, unsigned int old)
{
	return __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(acc, 4096.0f, 0x1p-13f), byte, old);
}

} // namespace vh
