// Part of colour.hip, which includes it (behind cbrt_exact.h and cbrt_quad.h): vips_sharpen for gfx950
// (convolution/sharpen.c) -- the LUT pass on a LabS image, and vips_sharpen of a whole uchar sRGB image (the LabS round
// trip, the blur of L and the LUT) in ONE kernel, in the tiers sharpen_fused_u8 picks from; their launchers, the C ABI.
#pragma once

#include "colour_device.h"
#include "colour_rows.h"

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

namespace vh {

struct SharpenArgs {
	const unsigned char *in, *blur;
	unsigned char *out;
	long long in_stride, blur_stride, out_stride;
	int width, height, bands;
	const int *lut;
};

// vips_sharpen_generate, sharpen.c:116-168, on band 0 of a LabS image; the other
// bands are copied (the reference splits them off and joins them back, :274-295).
__global__ void __launch_bounds__(256)
sharpen_kernel(SharpenArgs a)
{
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= a.width)
		return;
	for (int y0 = blockIdx.y * RU; y0 < a.height; y0 += gridDim.y * RU) {
		int v1[RU], v2[RU];
#pragma unroll
		for (int r = 0; r < RU; r++) {
			const int y = min(y0 + r, a.height - 1);
			v1[r] = ((const short *) (a.in + (long long) y * a.in_stride))[(long long) x * a.bands];
			v2[r] = ((const short *) (a.blur + (long long) y * a.blur_stride))[x];
		}
#pragma unroll
		for (int r = 0; r < RU; r++) {
			const int y = y0 + r;
			if (y < a.height) {
				const short *p1 = (const short *) (a.in + (long long) y * a.in_stride) + (long long) x * a.bands;
				short *q = (short *) (a.out + (long long) y * a.out_stride) + (long long) x * a.bands;
				const int diff = (v1[r] & 0x7fff) - (v2[r] & 0x7fff);
				int out = v1[r] + a.lut[diff + 32768];
				out = min(max(out, 0), 32767);
				q[0] = (short) out;
				for (int b = 1; b < a.bands; b++)
					q[b] = p1[b];
			}
		}
	}
}


// ------------------------------------------------- vips_sharpen on sRGB uchar, one kernel
//
// vips_sharpen (sharpen.c:171-302) on a 3-band uchar sRGB image is six operations on a small
// image -- colourspace(LABS), extract L, convsep of a 3..5-tap integer gaussian (two passes),
// the LUT step (sharpen.c:116-168), colourspace(sRGB) -- each a kernel that is over before the
// launch latency is (BASELINE config 4: 0.06 ms of the 0.14 ms per thumbnail).  Here a block
// owns a 64 x 32 (or 64 x 16) pixel tile: it converts the tile and its halo to LabS into LDS (route code of
// colour_device.h, image edges clamped = the embed of the convolution), runs the horizontal
// and the vertical pass on L in LDS with the convi C-path arithmetic and its rounding to short
// between the passes ((sum + scale / 2) / scale, C division: convi.c:698-716), applies the LUT
// and converts back: one read of the image, one write.
constexpr int SF_TW = 64, SF_MAXHALF = 2;
constexpr int SF_RW = SF_TW + 2 * SF_MAXHALF;

constexpr int SF_MAXB = 64; // images per launch

// the images of a launch (blockIdx.z), read where they lie in the kernarg segment
struct SharpenFusedPtrs {
	const unsigned char *in[SF_MAXB];
	unsigned char *out[SF_MAXB];
};

struct SharpenFusedArgs {
	long long in_stride, out_stride;
	int width, height;
	int n, half;          // blur taps, n / 2
	int coef[2 * SF_MAXHALF + 1];
	int scale, rounding;
	unsigned int magic;   // n / scale = (t + ((n - t) >> 1)) >> shift with t = mulhi(magic, n), 0 <= n < 2^32
	int shift;            // (Granlund & Montgomery's round-up multiplier; scale > 1)
	const int *lut;       // 65536 ints (sharpen.c:230-257)
	int zero_lo, zero_hi; // SKIP: lut[diff + 32768] == 0 for zero_lo <= diff <= zero_hi (empty: lo > hi)
	// SKIP: n / scale == ((n << sh24) * m24) >> 32 for every n a blur sum can be, both factors below 2^24 (the
	// full-rate v_mul_hi_u32_u24 instead of the quarter-rate v_mul_hi_u32; the host tried every n); sh24 < 0: no
	unsigned int m24;
	int sh24;
	// SKIP on large images (round 6): a tile whose list is longer than defer_threshold is left to the all-in-LDS
	// kernel -- its 64 x 64 tile goes on a device-side list (defer[0] the count, then one flag per such tile, then
	// the list) that sharpen_quad_u8_kernel walks afterwards; nullptr: every tile is finished here
	int *defer;
	int defer_threshold, q_tiles_x, q_tiles_y;
	int defer_raw;     // > 0: the tile is judged by its middle row's raw bytes (green of neighbours more than this apart)
	ColourTables tables;
};

static __device__ __forceinline__ int sf_convi_fin(int sum, const SharpenFusedArgs &a)
{
	// ((sum + rounding) / scale) with C (truncating) division, offset 0, clip to short.  The
	// divisor is the same for the whole launch: a multiply-high and two shifts on the magnitude
	// instead of the ~30 instructions of a 32-bit division
	const int x = sum + a.rounding;
	const unsigned int n = (unsigned int) (x < 0 ? -x : x);
	unsigned int m = n;
	if (a.scale != 1) {
		const unsigned int t = __umulhi(a.magic, n);
		m = (t + ((n - t) >> 1)) >> a.shift;
	}
	const int q = x < 0 ? -(int) m : (int) m;
	return min(max(q, -32768), 32767);
}

// the same for a sum that is not negative (the SKIP kernel: L >= 0, coefficients >= 0): n = sum + rounding < 2^31
static __device__ __forceinline__ unsigned int sf_div_nonneg(unsigned int n, const SharpenFusedArgs &a)
{
	// (the SKIP kernel is only launched with sh24 >= 0)
	unsigned int m;
	VH_MUL_HI_U24(m, n << a.sh24, a.m24);
	return min(m, 32767u);
}

// SF_TH = rows of a tile: 16 rows per pass of the block's 256 threads (4 pixels each), SF_TH / 16
// passes; the halo ring and the tables a block loads are shared by all of them
//
// SKIP (round 6): the pixels sharpen leaves alone skip the way back.  With the default parameters (m1 = 0) the
// LUT is 0 for |L - blur| < x1 = 2 L units (sharpen.c:230-257) -- every pixel of a smooth region: 95.7 % of the
// pixels of BASELINE config 4's thumbnails, most of a photograph.  Such a pixel leaves vips_sharpen as
// sRGB(LabS(pixel)) with L, a, b untouched, and sRGB -> LabS -> sRGB is the IDENTITY on all 2^24 colours: checked
// with the compiled reference on the host (tests/test_oracle_conv_colour.py) and, for the device's own tables and
// these very functions, exhaustively on the device before the first launch (sharpen_identity_kernel: the kernel is
// only selected when the count of colours that do not come back is 0).  So: L alone (not a, b: a third of the
// forward path's table reads) for the tile and its halo, the blur, the test of L - blur against the LUT's zero
// window (no gather); the tile's INPUT bytes wait in LDS as its output; the few pixels whose LUT entry is not 0
// are appended to a list (LDS atomic), taken through the full forward and backward path DENSELY (a wave of list
// entries, not a wave of tile pixels 4 % of which are live) and patched into the staged bytes.
// (NT = taps the SKIP kernel's blur passes compute: 3 or 5; the other kernel always runs five, zeros included)
// (a flag another kernel of the stream wrote: the same for every lane)
static __device__ __forceinline__ int uniform_flag(const int *p)
{
	return __builtin_amdgcn_readfirstlane(*p);
}

// Large images, before sharpen_fused_u8_kernel<32, true>: which tiles are noise or dense edges -- the all-in-LDS
// kernel's anyway -- judged from the raw bytes of ONE row: a THREAD per 64 x 32 tile walks its middle row and counts
// the horizontal neighbours whose green differs by more than `raw`; more than half: the tile's 64 x 64 parent goes on
// the device-side list (SharpenFusedArgs::defer) and both kernels know.  A heuristic for speed only: both kernels make
// the same pixels.  The list's slots are handed out a wave at a time (one atomic on the counter per wave that has any):
// round 6's first form judged inside the skip kernel, a block a tile, and what a noisy 8192 x 8192 image paid 0.19 ms
// for was 16 384 atomics on ONE counter -- measured again with a wave a tile in this kernel: the same 0.19 ms.
__global__ void __launch_bounds__(256)
sharpen_survey_kernel(SharpenFusedPtrs ptrs_by_value, int width, int height, long long in_stride, int raw, int *defer,
	int q_tiles_x, int q_tiles_y, int tiles_x, int tiles_y)
{
	__shared__ int s_base[4];
	(void) ptrs_by_value;
	typedef const unsigned long long __attribute__((address_space(4))) *KernargPtrs;
	const KernargPtrs kp = (KernargPtrs) __builtin_amdgcn_kernarg_segment_ptr();
	typedef const unsigned char __attribute__((address_space(1))) *GlobalIn;
	const GlobalIn in = (GlobalIn) kp[blockIdx.z];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int tile = (int) blockIdx.x * 256 + (int) threadIdx.x;
	const bool valid = tile < tiles_x * tiles_y;
	const int tc = valid ? tile : 0;
	const int ty = tc / tiles_x, tx = tc - ty * tiles_x;
	const int x0 = tx * SF_TW, y0 = ty * 32;
	const int ym = min(y0 + 16, height - 1);
	const GlobalIn row = in + (long long) ym * in_stride;
	int count = 0;
	int prev = row[3 * x0 + 1];
	for (int j = 1; j <= SF_TW; j++) {
		const int g = row[3 * min(x0 + j, width - 1) + 1];
		count += (x0 + j - 1 < width && abs(g - prev) > raw) ? 1 : 0;
		prev = g;
	}
	const int per = q_tiles_x * q_tiles_y;
	const int qt = (int) blockIdx.z * per + (y0 / 64) * q_tiles_x + tx;
	const int total = per * (int) gridDim.z;
	bool fresh = false;
	if (valid && count > SF_TW / 2)
		fresh = atomicExch(defer + 1 + qt, 1) == 0; // (a 64 x 64 parent has two tiles: the first one lists it)
	const unsigned long long mask = __builtin_amdgcn_ballot_w64(fresh);
	const int n = __builtin_popcountll(mask);
	const int rank = __builtin_popcountll(mask & ((1ULL << lane) - 1ULL));
	if (lane == 0 && n)
		s_base[wave] = atomicAdd(defer, n);
	__syncthreads();
	if (fresh)
		defer[1 + total + s_base[wave] + rank] = qt;
}

template <int SF_TH, bool SKIP, int NT = 2 * SF_MAXHALF + 1>
__global__ void __launch_bounds__(256)
sharpen_fused_u8_kernel(SharpenFusedPtrs ptrs_by_value, SharpenFusedArgs a)
{
	constexpr int SF_RH = SF_TH + 2 * SF_MAXHALF;
	constexpr int NCH = SKIP ? 1 : 3;
	constexpr int OUT_DW = SF_TW * 3 / 4; // dwords per staged row
	__shared__ __attribute__((aligned(16))) short s_lab[SF_RH][SF_RW][NCH];
	__shared__ __attribute__((aligned(16))) short s_h[SF_RH][SF_TW];
	// the two 8-bit colour tables in LDS: six of a pixel's table reads stay off the vector memory path
	__shared__ float s_v2Y[256];
	__shared__ int s_Y2v[260];
	__shared__ unsigned int s_out[SKIP ? SF_TH * OUT_DW : 1];  // SKIP: the tile's bytes, input until patched
	__shared__ unsigned int s_list[SKIP ? SF_TH * SF_TW : 1];  // SKIP: (LUT index << 11) | row << 6 | column
	__shared__ int s_count;
	(void) ptrs_by_value;
	typedef const unsigned long long __attribute__((address_space(4))) *KernargPtrs;
	const KernargPtrs kp = (KernargPtrs) __builtin_amdgcn_kernarg_segment_ptr();
	// (pointers made from integers are generic to the compiler: say they are global)
	typedef const unsigned char __attribute__((address_space(1))) *GlobalIn;
	typedef unsigned char __attribute__((address_space(1))) *GlobalOut;
	const GlobalIn in = (GlobalIn) kp[blockIdx.z];
	const GlobalOut out = (GlobalOut) kp[SF_MAXB + blockIdx.z];
	const int t = threadIdx.x;
	const int x0 = blockIdx.x * SF_TW, y0 = blockIdx.y * SF_TH;
	const int h = a.half;
	const int rw = SF_TW + 2 * h, rh = SF_TH + 2 * h;
	if constexpr (SKIP) {
		if (a.defer && a.defer_raw > 0) {
			// 0' (large images only): sharpen_survey_kernel has judged every tile already; one that is on the list is
			// the all-in-LDS kernel's -- leave before the block has touched anything
			const int per = a.q_tiles_x * a.q_tiles_y;
			const int qt = (int) blockIdx.z * per + (y0 / 64) * a.q_tiles_x + (int) blockIdx.x;
			if (uniform_flag(a.defer + 1 + qt))
				return;
		}
	}
	s_v2Y[threadIdx.x] = a.tables.v2Y_8[threadIdx.x];
	s_Y2v[threadIdx.x] = a.tables.Y2v_8[threadIdx.x];
	if (threadIdx.x == 0) {
		s_Y2v[256] = a.tables.Y2v_8[256];
		s_count = 0;
	}
	__syncthreads();

	// ring pixel idx -> its place in the region (the frame of h pixels around the tile)
	auto ring_place = [&](int idx, int &ry, int &rx) {
		if (idx < 2 * rw * h) {
			// rows above and below (h <= 2: at most four rows, no division)
			const int r = (idx >= rw) + (idx >= 2 * rw) + (idx >= 3 * rw);
			rx = idx - r * rw;
			ry = r < h ? r : SF_TH + r;
		}
		else {
			// columns left and right of the tile's rows (2 h = 2 or 4 = 1 << h)
			const int k = idx - 2 * rw * h;
			const int r = k >> h, c = k & (2 * h - 1);
			ry = h + r;
			rx = c < h ? c : SF_TW + c;
		}
	};
	if constexpr (SKIP) {
		if (a.defer && a.defer_raw <= 0) {
			// 0 (large images only; $VIPS_HIP_SHARPEN_DEFER_RAW=0). A tile of noise or dense edges goes to the all-in-LDS kernel anyway: find out
			// from ONE row before paying for all of them -- L of the tile's middle row and the rows either side, the
			// blur of the middle row, its pixels outside the LUT's zero window counted; more than half: the tile is
			// deferred here and now.  (A heuristic for speed only: both kernels make the same pixels.)
			const int ym = min(y0 + SF_TH / 2, a.height - 1);
			const int nrow = 2 * h + 1;
			for (int idx = t; idx < nrow * rw; idx += 256) {
				const int rr = idx / rw, rx = idx - rr * rw;
				const int x = min(max(x0 + rx - h, 0), a.width - 1);
				const int y = min(max(ym + rr - h, 0), a.height - 1);
				unsigned int off;
				VH_MAD_U24(off, (unsigned int) y, (unsigned int) a.in_stride, (unsigned int) (3 * x));
				const GlobalIn p = in + off;
				short L, A = 0, B = 0;
				srgb8_to_labs<false>(a.tables, s_v2Y, p[0], p[1], p[2], L, A, B);
				s_lab[rr][rx][0] = L;
			}
			__syncthreads();
			for (int idx = t; idx < nrow * SF_TW; idx += 256) {
				const int rr = idx >> 6, cx = idx & 63;
				unsigned int sum = (unsigned int) a.rounding;
#pragma unroll
				for (int k = 0; k < NT; k++)
					VH_MAD_U24(sum, (unsigned int) (int) s_lab[rr][cx + k][0], (unsigned int) a.coef[k], sum);
				s_h[rr][cx] = (short) sf_div_nonneg(sum, a);
			}
			__syncthreads();
			if (t < SF_TW) {
				unsigned int sum = (unsigned int) a.rounding;
#pragma unroll
				for (int k = 0; k < NT; k++)
					VH_MAD_U24(sum, (unsigned int) (int) s_h[k][t], (unsigned int) a.coef[k], sum);
				const int blur = (int) sf_div_nonneg(sum, a);
				const int v1 = s_lab[h][t + h][0];
				const int diff = (v1 & 0x7fff) - (blur & 0x7fff);
				if ((diff < a.zero_lo || diff > a.zero_hi) && x0 + t < a.width)
					atomicAdd(&s_count, 1);
			}
			__syncthreads();
			const int sampled = s_count;
			__syncthreads();
			if (sampled > SF_TW / 2) {
				if (t == 0) {
					const int per = a.q_tiles_x * a.q_tiles_y;
					const int qt = (int) blockIdx.z * per + (y0 / 64) * a.q_tiles_x + (int) blockIdx.x;
					const int total = per * (int) gridDim.z;
					if (atomicExch(a.defer + 1 + qt, 1) == 0)
						a.defer[1 + total + atomicAdd(a.defer, 1)] = qt;
				}
				return;
			}
			if (t == 0)
				s_count = 0;
			// (the barrier in front of sweep 3's LDS writes orders this; s_lab / s_h rows 0 .. 2 are written anew)
			__syncthreads();
		}
		// 1 (SKIP). L of the tile and its ring, IN THREE SWEEPS over the thread's pixels (4 per 16 rows of the tile
		// and up to two of the ring): every pixel load, then every table index and its gather, then the
		// interpolations -- two memory latencies a block instead of two per pixel group (the block's life is those
		// latencies: with the conversions one after the other the kernel ran no faster for 40 % fewer instructions)
		constexpr int NPASS = SF_TH / 16, NRING = 2, NPX = 4 * NPASS + NRING;
		const int ring = rw * rh - SF_TW * SF_TH;
		const int quad = t & 15;
		const bool words = !((((unsigned long long) in) | (unsigned long long) a.in_stride) & 3) && x0 + 4 * quad + 4 <= a.width;
		unsigned int w[NPASS][3];
		unsigned int rpx[NRING][3];
		int rry[NRING], rrx[NRING];
#pragma unroll
		for (int pass = 0; pass < NPASS; pass++) {
			const int row = (t >> 4) + 16 * pass;
			const int y = min(y0 + row, a.height - 1);
			const int x = x0 + 4 * quad;
			unsigned int off;
			VH_MAD_U24(off, (unsigned int) y, (unsigned int) a.in_stride, 0u);
			const GlobalIn line = in + off;
			if (words) {
				const unsigned int __attribute__((address_space(1))) *p4 =
					(const unsigned int __attribute__((address_space(1))) *) (line + 3 * x);
#pragma unroll
				for (int k = 0; k < 3; k++)
					w[pass][k] = p4[k];
			}
			else {
				unsigned char px[12];
#pragma unroll
				for (int m = 0; m < 4; m++) {
					const GlobalIn p = line + 3 * min(x + m, a.width - 1);
					px[3 * m] = p[0];
					px[3 * m + 1] = p[1];
					px[3 * m + 2] = p[2];
				}
#pragma unroll
				for (int k = 0; k < 3; k++)
					w[pass][k] = (unsigned) px[4 * k] | ((unsigned) px[4 * k + 1] << 8) | ((unsigned) px[4 * k + 2] << 16) |
						((unsigned) px[4 * k + 3] << 24);
			}
		}
#pragma unroll
		for (int j = 0; j < NRING; j++) {
			const int idx = min(t + 256 * j, ring - 1); // (a lane beyond the ring repeats its last pixel: same value, same place)
			ring_place(max(idx, 0), rry[j], rrx[j]);
			const int x = min(max(x0 + rrx[j] - h, 0), a.width - 1);
			const int y = min(max(y0 + rry[j] - h, 0), a.height - 1);
			unsigned int off;
			VH_MAD_U24(off, (unsigned int) y, (unsigned int) a.in_stride, (unsigned int) (3 * x));
			const GlobalIn p = in + off;
			rpx[j][0] = p[0];
			rpx[j][1] = p[1];
			rpx[j][2] = p[2];
		}
		// sweep 2: Y of every pixel, its table index and fraction, the gather
		float fr[NPX];
		float2 pair[NPX];
		auto index_of = [&](int n, unsigned int r8, unsigned int g8, unsigned int b8) {
			Px v;
			v.a = s_v2Y[r8];
			v.b = s_v2Y[g8];
			v.c = s_v2Y[b8];
			v = step_scRGB2XYZ(v);
			const int i = cbrt_index_finite<1>(v.b, fr[n]);
			__builtin_memcpy(&pair[n], a.tables.cbrt + i, sizeof(float2));
		};
#pragma unroll
		for (int pass = 0; pass < NPASS; pass++)
#pragma unroll
			for (int m = 0; m < 4; m++) {
				// byte 3 m + c of the 12: dword (3 m + c) / 4, byte (3 m + c) % 4
				auto byte_of = [&](int c) -> unsigned int { return (w[pass][(3 * m + c) >> 2] >> (8 * ((3 * m + c) & 3))) & 0xffu; };
				index_of(4 * pass + m, byte_of(0), byte_of(1), byte_of(2));
			}
#pragma unroll
		for (int j = 0; j < NRING; j++)
			index_of(4 * NPASS + j, rpx[j][0], rpx[j][1], rpx[j][2]);
		// sweep 3: interpolate, L, LabS (the operations of srgb8_to_labs<false>, in its order)
		auto finish = [&](int n) -> short {
			const float cby = cbrt_finish(pair[n], fr[n]);
			return lab2labs_finite(__fsub_rn(__fmul_rn(116.0F, cby), 16.0F), 32767.0 / 100.0, 0.0);
		};
#pragma unroll
		for (int pass = 0; pass < NPASS; pass++) {
			const int row = (t >> 4) + 16 * pass;
#pragma unroll
			for (int m = 0; m < 4; m++)
				s_lab[row + h][4 * quad + m + h][0] = finish(4 * pass + m);
#pragma unroll
			for (int k = 0; k < 3; k++)
				s_out[row * OUT_DW + 3 * quad + k] = w[pass][k];
		}
#pragma unroll
		for (int j = 0; j < NRING; j++)
			if (t + 256 * j < ring)
				s_lab[rry[j]][rrx[j]][0] = finish(4 * NPASS + j);
	}
	else {
	// 1. the tile and its halo: sRGB uchar -> LabS.
	// 1a. the tile itself, 4 pixels per thread (the mapping of step 3): 12 bytes as three dwords
	// when the row allows it, the four conversions side by side (their table reads overlap)
	for (int pass = 0; pass < SF_TH / 16; pass++) {
		const int row = (t >> 4) + 16 * pass, quad = t & 15;
		const int y = min(y0 + row, a.height - 1);
		const int x = x0 + 4 * quad;
		const GlobalIn line = in + (long long) y * a.in_stride;
		unsigned char px[12];
		if (x + 4 <= a.width && !((((unsigned long long) in) | (unsigned long long) a.in_stride) & 3)) {
			const unsigned int __attribute__((address_space(1))) *p4 =
				(const unsigned int __attribute__((address_space(1))) *) (line + 3LL * x);
#pragma unroll
			for (int w = 0; w < 3; w++) {
				const unsigned int v = p4[w];
				px[4 * w] = (unsigned char) v;
				px[4 * w + 1] = (unsigned char) (v >> 8);
				px[4 * w + 2] = (unsigned char) (v >> 16);
				px[4 * w + 3] = (unsigned char) (v >> 24);
			}
		}
		else {
#pragma unroll
			for (int m = 0; m < 4; m++) {
				const GlobalIn p = line + 3LL * min(x + m, a.width - 1);
				px[3 * m] = p[0];
				px[3 * m + 1] = p[1];
				px[3 * m + 2] = p[2];
			}
		}
#pragma unroll
		for (int m = 0; m < 4; m++) {
			short L, A = 0, B = 0;
			srgb8_to_labs<!SKIP>(a.tables, s_v2Y, px[3 * m], px[3 * m + 1], px[3 * m + 2], L, A, B);
			s_lab[row + h][4 * quad + m + h][0] = L;
			if constexpr (!SKIP) {
				s_lab[row + h][4 * quad + m + h][1] = A;
				s_lab[row + h][4 * quad + m + h][2] = B;
			}
		}
		if constexpr (SKIP) {
#pragma unroll
			for (int w = 0; w < 3; w++)
				s_out[row * OUT_DW + 3 * quad + w] = (unsigned) px[4 * w] | ((unsigned) px[4 * w + 1] << 8) |
					((unsigned) px[4 * w + 2] << 16) | ((unsigned) px[4 * w + 3] << 24);
		}
	}
	// 1b. the ring of h pixels around it (image edges clamped): only L is blurred, so only L
	{
		const int ring = rw * rh - SF_TW * SF_TH;
		for (int idx = t; idx < ring; idx += 256) {
			int ry, rx;
			ring_place(idx, ry, rx);
			const int x = min(max(x0 + rx - h, 0), a.width - 1);
			const int y = min(max(y0 + ry - h, 0), a.height - 1);
			GlobalIn p;
			if constexpr (SKIP) {
				// (the host keeps height * stride below 2^31 and both factors below 2^24 for this kernel)
				unsigned int off;
				VH_MAD_U24(off, (unsigned int) y, (unsigned int) a.in_stride, (unsigned int) (3 * x));
				p = in + off;
			}
			else
				p = in + (long long) y * a.in_stride + 3LL * x;
			short L, A = 0, B = 0;
			srgb8_to_labs<false>(a.tables, s_v2Y, p[0], p[1], p[2], L, A, B);
			s_lab[ry][rx][0] = L;
		}
	}
		}
	__syncthreads();
	// 2. horizontal pass on L (all rows of the region, the tile's columns)
	if constexpr (SKIP) {
		// four neighbouring outputs per thread from ONE read of their 8 shorts (rows are 8-byte aligned); L and the
		// coefficients are not negative here (host), so a sum is not and its division is the multiply-high alone
		for (int item = t; item < rh * (SF_TW / 4); item += 256) {
			const int ry = item >> 4, q4 = (item & 15) * 4;
			const uint2 w0 = *reinterpret_cast<const uint2 *>(&s_lab[ry][q4][0]);
			const uint2 w1 = *reinterpret_cast<const uint2 *>(&s_lab[ry][q4 + 4][0]);
			const int v[8] = { (int) (w0.x & 0xffffu), (int) (w0.x >> 16), (int) (w0.y & 0xffffu), (int) (w0.y >> 16),
				(int) (w1.x & 0xffffu), (int) (w1.x >> 16), (int) (w1.y & 0xffffu), (int) (w1.y >> 16) };
			unsigned int o[4];
#pragma unroll
			for (int m = 0; m < 4; m++) {
				unsigned int sum = (unsigned int) a.rounding;
#pragma unroll
				for (int k = 0; k < NT; k++)
					VH_MAD_U24(sum, (unsigned int) v[m + k], (unsigned int) a.coef[k], sum);
				o[m] = sf_div_nonneg(sum, a);
			}
			*reinterpret_cast<uint2 *>(&s_h[ry][q4]) = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
		}
	}
	else {
		for (int idx = t; idx < rh * SF_TW; idx += 256) {
			const int ry = idx / SF_TW, cx = idx - ry * SF_TW;
			// always five taps (coefficients beyond the mask are zero, the reads stay inside the arrays)
			int sum = 0;
#pragma unroll
			for (int k = 0; k < 2 * SF_MAXHALF + 1; k++)
				sum += a.coef[k] * (int) s_lab[ry][cx + k][0];
			s_h[ry][cx] = (short) sf_convi_fin(sum, a);
		}
	}
	__syncthreads();
	// 3. vertical pass, the LUT, back to sRGB: 4 pixels per thread, three dword stores
	for (int pass = 0; pass < SF_TH / 16; pass++) {
		const int row = (t >> 4) + 16 * pass, quad = t & 15;
		const int y = y0 + row;
		if constexpr (SKIP) {
			if (y >= a.height)
				continue;
			// the thread's four columns of the 2 h + 1 rows above and below: one 8-byte read per row
			unsigned int sum[4] = { (unsigned int) a.rounding, (unsigned int) a.rounding, (unsigned int) a.rounding,
				(unsigned int) a.rounding };
#pragma unroll
			for (int k = 0; k < NT; k++) {
				const uint2 w = *reinterpret_cast<const uint2 *>(&s_h[row + k][4 * quad]);
				const unsigned int ck = (unsigned int) a.coef[k];
				VH_MAD_U24(sum[0], w.x & 0xffffu, ck, sum[0]);
				VH_MAD_U24(sum[1], w.x >> 16, ck, sum[1]);
				VH_MAD_U24(sum[2], w.y & 0xffffu, ck, sum[2]);
				VH_MAD_U24(sum[3], w.y >> 16, ck, sum[3]);
			}
			// inside the LUT's zero window: the staged input bytes are the result.  The others go on the list with
			// their LUT index (the LUT itself is read in step 4: no memory latency here), one LDS atomic per thread
			unsigned int entry[4];
			int n_mine = 0;
#pragma unroll
			for (int m = 0; m < 4; m++) {
				const int cx = 4 * quad + m;
				const int blur = (int) sf_div_nonneg(sum[m], a);
				const int v1 = s_lab[row + h][cx + h][0];
				const int diff = (v1 & 0x7fff) - (blur & 0x7fff);
				const bool live = (diff < a.zero_lo || diff > a.zero_hi) && x0 + cx < a.width;
				entry[m] = live ? ((unsigned) (diff + 32768) << 11) | (unsigned) (row * SF_TW + cx) : 0xffffffffu;
				n_mine += live ? 1 : 0;
			}
			if (n_mine > 0) {
				int at = atomicAdd(&s_count, n_mine);
#pragma unroll
				for (int m = 0; m < 4; m++)
					if (entry[m] != 0xffffffffu)
						s_list[at++] = entry[m];
			}
			continue;
		}
		if (y < a.height) {
			unsigned char o[12];
#pragma unroll
			for (int m = 0; m < 4; m++) {
				const int cx = 4 * quad + m;
				int sum = 0;
#pragma unroll
				for (int k = 0; k < 2 * SF_MAXHALF + 1; k++)
					sum += a.coef[k] * (int) s_h[row + k][cx];
				const int blur = sf_convi_fin(sum, a);
				const int v1 = s_lab[row + h][cx + h][0];
				const int diff = (v1 & 0x7fff) - (blur & 0x7fff);
				int sharp = v1 + a.lut[diff + 32768];
				sharp = min(max(sharp, 0), 32767);
				labs_to_srgb8(s_Y2v, sharp, s_lab[row + h][cx + h][1], s_lab[row + h][cx + h][2], o[3 * m],
					o[3 * m + 1], o[3 * m + 2]);
			}
			const int x = x0 + 4 * quad;
			const GlobalOut dst = out + (long long) y * a.out_stride + 3LL * x;
			if (x + 4 <= a.width && !(((uintptr_t) dst) & 3)) {
				unsigned int __attribute__((address_space(1))) *d4 = (unsigned int __attribute__((address_space(1))) *) dst;
#pragma unroll
				for (int w = 0; w < 3; w++)
					d4[w] = (unsigned) o[4 * w] | ((unsigned) o[4 * w + 1] << 8) | ((unsigned) o[4 * w + 2] << 16) |
						((unsigned) o[4 * w + 3] << 24);
			}
			else {
				for (int m = 0; m < 12 && x + m / 3 < a.width; m++)
					dst[m] = o[m];
			}
		}
	}
	if constexpr (SKIP) {
		// 4. the listed pixels, densely: forward for a, b, back from (sharpened L, a, b), patched into the stage
		__syncthreads();
		const int count = s_count;
		if (a.defer && count > a.defer_threshold) {
			// mostly edges or noise: the kernel with every table in LDS does such a tile faster (the whole 64 x 64
			// tile this one is a half of; its other half may finish here: the same pixels either way)
			if (t == 0) {
				const int per = a.q_tiles_x * a.q_tiles_y;
				const int qt = (int) blockIdx.z * per + (y0 / 64) * a.q_tiles_x + (int) blockIdx.x;
				const int total = per * (int) gridDim.z;
				if (atomicExch(a.defer + 1 + qt, 1) == 0)
					a.defer[1 + total + atomicAdd(a.defer, 1)] = qt;
			}
			return;
		}
		unsigned char *bytes = reinterpret_cast<unsigned char *>(s_out);
		for (int i = t; i < count; i += 256) {
			const unsigned int e = s_list[i];
			const int pos = (int) (e & 2047u);
			const int add = a.lut[e >> 11]; // sharpen.c:116-168: index (v1 & 0x7fff) - (blur & 0x7fff) + 32768
			if (add == 0)
				continue; // (a zero of the LUT outside the window around 0: the staged bytes stand)
			const int row = pos / SF_TW, cx = pos - row * SF_TW;
			const int sharp = min(max((int) s_lab[row + h][cx + h][0] + add, 0), 32767);
			unsigned char *p = bytes + row * (OUT_DW * 4) + 3 * cx;
			short L, A, B;
			srgb8_to_labs<true>(a.tables, s_v2Y, p[0], p[1], p[2], L, A, B);
			unsigned char r8, g8, b8;
			labs_to_srgb8(s_Y2v, sharp, A, B, r8, g8, b8);
			p[0] = r8;
			p[1] = g8;
			p[2] = b8;
		}
		__syncthreads();
		// 5. the stage leaves: 4 pixels per thread, three dword stores
		for (int pass = 0; pass < SF_TH / 16; pass++) {
			const int row = (t >> 4) + 16 * pass, quad = t & 15;
			const int y = y0 + row;
			if (y >= a.height)
				continue;
			const int x = x0 + 4 * quad;
			const GlobalOut dst = out + (long long) y * a.out_stride + 3LL * x;
			const unsigned int *src = s_out + row * OUT_DW + 3 * quad;
			if (x + 4 <= a.width && !(((uintptr_t) dst) & 3)) {
				unsigned int __attribute__((address_space(1))) *d4 = (unsigned int __attribute__((address_space(1))) *) dst;
#pragma unroll
				for (int w = 0; w < 3; w++)
					d4[w] = src[w];
			}
			else {
				const unsigned char *sb = reinterpret_cast<const unsigned char *>(src);
				for (int m = 0; m < 12 && x + m / 3 < a.width; m++)
					dst[m] = sb[m];
			}
		}
	}
}

// sRGB -> LabS -> sRGB with the functions above on every one of the 2^24 colours: the count of colours that do not
// come back.  0 is what lets sharpen_fused_u8_kernel<*, true> hand a pixel whose LUT entry is 0 through untouched.
__global__ void __launch_bounds__(256)
sharpen_identity_kernel(ColourTables tables, unsigned int *bad)
{
	__shared__ float s_v2Y[256];
	__shared__ int s_Y2v[260];
	s_v2Y[threadIdx.x] = tables.v2Y_8[threadIdx.x];
	s_Y2v[threadIdx.x] = tables.Y2v_8[threadIdx.x];
	if (threadIdx.x == 0)
		s_Y2v[256] = tables.Y2v_8[256];
	__syncthreads();
	const unsigned int c = blockIdx.x * 256u + threadIdx.x;
	const int r = (int) (c >> 16), g = (int) ((c >> 8) & 255u), b = (int) (c & 255u);
	short L, A, B;
	srgb8_to_labs<true>(tables, s_v2Y, r, g, b, L, A, B);
	unsigned char r8, g8, b8;
	// (the kernel's clip of L + 0 to 0 .. 32767 is part of what is checked)
	labs_to_srgb8(s_Y2v, min(max((int) L, 0), 32767), A, B, r8, g8, b8);
	if (r8 != r || g8 != g || b8 != b)
		atomicAdd(bad, 1u);
}

// ------------------------------------------------- ... with every table in LDS (round 5)
//
// sharpen_fused_u8 reads four tables per pixel through global memory (XYZ2Lab's 400 KB cube-root table three
// times, sharpen's 256 KB LUT once) and a wave's gather from an L2-resident table takes ~146 cycles of its CU's
// L1 fill path (tools/gather_probe.hip): 4 x 146 cycles per 64 pixels IS the kernel's 1.06 ms on 8192^2.  Here a
// block of 1024 threads copies everything it looks up into LDS once and then walks tiles of 64 x 64 pixels:
//   * the cube-root table in cbrt_quad.h's form (57 KB, ~27 instructions and two LDS reads per pair);
//   * the part of sharpen's LUT that is not constant (sharpen.c:230-257 is flat outside a few thousand entries
//     round the middle: the host finds the window; a LUT with a wider one takes the older kernel);
//   * the two 8-bit sRGB tables.
// Same steps, same roundings as the older kernel (colour_device.h); one block per CU (106 KB of LDS, 16 waves).
constexpr int SQ_NT = 1024, SQ_T = 64, SQ_R = SQ_T + 2 * SF_MAXHALF;
constexpr int SQ_MAXLUT = 6144; // entries of the LUT's window

struct SharpenQuadArgs {
	SharpenFusedArgs f;
	CbrtQuad cq;
	const short *lut_win; // lut_n entries from index lut_lo
	int lut_lo, lut_n, lut_below, lut_above;
	int tiles_x, tiles_y, n_images;
	const int *defer; // list mode (see SharpenFusedArgs::defer): the tiles sharpen_fused_u8_kernel<*, true> left; else nullptr
};

// XYZ2Lab.c:109-138 on a small finite value: the table pair from LDS
static __device__ __forceinline__ float sq_cbrt(const CbqBlock *blk, const unsigned int *res, float n)
{
	const int i = min(max(vh::cvt_i32(n), 0), CBRT_N - 2);
	const float fi = (float) i;
	float t0, dt;
	cbq_pair(blk, res, i, fi, &t0, &dt);
	return __fadd_rn(t0, __fmul_rn(__fsub_rn(n, fi), dt));
}

template <bool WANT_AB>
static __device__ __forceinline__ void sq_to_labs(const CbqBlock *blk, const unsigned int *res, const float *v2Y, int r, int g,
	int b, short &L, short &A, short &B)
{
	Px v;
	v.a = v2Y[r];
	v.b = v2Y[g];
	v.c = v2Y[b];
	v = step_scRGB2XYZ(v);
	const float cby = sq_cbrt(blk, res, quant_div_finite<1>(__fmul_rn(100000.0f, v.b)));
	L = lab2labs_finite(__fsub_rn(__fmul_rn(116.0F, cby), 16.0F), 32767.0 / 100.0, 0.0);
	if (WANT_AB) {
		const float cbx = sq_cbrt(blk, res, quant_div_finite<0>(__fmul_rn(100000.0f, v.a)));
		const float cbz = sq_cbrt(blk, res, quant_div_finite<2>(__fmul_rn(100000.0f, v.c)));
		A = lab2labs_finite(__fmul_rn(500.0F, __fsub_rn(cbx, cby)), 32768.0 / 128.0, -32768.0);
		B = lab2labs_finite(__fmul_rn(200.0F, __fsub_rn(cby, cbz)), 32768.0 / 128.0, -32768.0);
	}
}

__global__ void __launch_bounds__(SQ_NT)
sharpen_quad_u8_kernel(SharpenFusedPtrs ptrs_by_value, SharpenQuadArgs q)
{
	VH_DYNAMIC_LDS(unsigned int, sq_lds);
	(void) ptrs_by_value;
	const SharpenFusedArgs &a = q.f;
	CbqBlock *const s_blk = reinterpret_cast<CbqBlock *>(sq_lds);
	unsigned int *const s_res = sq_lds + CBQ_BLOCKS * 4;
	float *const s_v2Y = reinterpret_cast<float *>(s_res + CBQ_RES_WORDS);
	int *const s_Y2v = reinterpret_cast<int *>(s_v2Y + 256);
	short *const s_lut = reinterpret_cast<short *>(s_Y2v + 260);
	short *const s_L = s_lut + SQ_MAXLUT + 8;                                   // [SQ_R][SQ_R]
	unsigned int *const s_ab = reinterpret_cast<unsigned int *>(s_L + SQ_R * SQ_R); // [SQ_T][SQ_T]: a | b << 16
	short *const s_h = reinterpret_cast<short *>(s_ab + SQ_T * SQ_T);            // [SQ_R][SQ_T]
	const int t = threadIdx.x;
	for (int i = t; i < CBQ_BLOCKS; i += SQ_NT)
		s_blk[i] = q.cq.blk[i];
	for (int i = t; i < CBQ_RES_WORDS; i += SQ_NT)
		s_res[i] = q.cq.res[i];
	if (t < 256)
		s_v2Y[t] = a.tables.v2Y_8[t];
	if (t < 257)
		s_Y2v[t] = a.tables.Y2v_8[t];
	for (int i = t; i < q.lut_n; i += SQ_NT)
		s_lut[i] = q.lut_win[i];
	typedef const unsigned long long __attribute__((address_space(4))) *KernargPtrs;
	const KernargPtrs kp = (KernargPtrs) __builtin_amdgcn_kernarg_segment_ptr();
	typedef const unsigned char __attribute__((address_space(1))) *GlobalIn;
	typedef unsigned char __attribute__((address_space(1))) *GlobalOut;
	const int h = a.half;
	const int rw = SQ_T + 2 * h;
	const int all_tiles = q.tiles_x * q.tiles_y * q.n_images;
	const int tiles = q.defer ? q.defer[0] : all_tiles;
	const int row = t >> 4, quad = t & 15;
	for (int ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
		const int tile = q.defer ? q.defer[1 + all_tiles + ti] : ti;
		const int img = tile / (q.tiles_x * q.tiles_y), tt = tile - img * (q.tiles_x * q.tiles_y);
		const int ty = tt / q.tiles_x, tx = tt - ty * q.tiles_x;
		const GlobalIn in = (GlobalIn) kp[img];
		const GlobalOut out = (GlobalOut) kp[SF_MAXB + img];
		const int x0 = tx * SQ_T, y0 = ty * SQ_T;
		__syncthreads(); // (the tables are there; the last tile's readers are done)
		// 1a. the tile: 4 pixels per thread -> LabS
		{
			const int y = min(y0 + row, a.height - 1);
			const int x = x0 + 4 * quad;
			const GlobalIn line = in + (long long) y * a.in_stride;
			unsigned char px[12];
			if (x + 4 <= a.width && !((((unsigned long long) in) | (unsigned long long) a.in_stride) & 3)) {
				const unsigned int __attribute__((address_space(1))) *p4 =
					(const unsigned int __attribute__((address_space(1))) *) (line + 3LL * x);
#pragma unroll
				for (int w = 0; w < 3; w++) {
					const unsigned int v = p4[w];
					px[4 * w] = (unsigned char) v;
					px[4 * w + 1] = (unsigned char) (v >> 8);
					px[4 * w + 2] = (unsigned char) (v >> 16);
					px[4 * w + 3] = (unsigned char) (v >> 24);
				}
			}
			else {
#pragma unroll
				for (int m = 0; m < 4; m++) {
					const GlobalIn p = line + 3LL * min(x + m, a.width - 1);
					px[3 * m] = p[0];
					px[3 * m + 1] = p[1];
					px[3 * m + 2] = p[2];
				}
			}
#pragma unroll
			for (int m = 0; m < 4; m++) {
				short L, A, B;
				sq_to_labs<true>(s_blk, s_res, s_v2Y, px[3 * m], px[3 * m + 1], px[3 * m + 2], L, A, B);
				s_L[(row + h) * SQ_R + 4 * quad + m + h] = L;
				s_ab[row * SQ_T + 4 * quad + m] = ((unsigned int) A & 0xffffu) | ((unsigned int) B << 16);
			}
		}
		// 1b. the ring of h pixels round it (image edges clamped): L only
		{
			const int ring = rw * rw - SQ_T * SQ_T;
			if (t < ring) {
				int ry, rx;
				if (t < 2 * rw * h) {
					const int r = t / rw;
					rx = t - r * rw;
					ry = r < h ? r : SQ_T + r;
				}
				else {
					const int k = t - 2 * rw * h;
					const int r = k / (2 * h), c = k - r * 2 * h;
					ry = h + r;
					rx = c < h ? c : SQ_T + c;
				}
				const int x = min(max(x0 + rx - h, 0), a.width - 1);
				const int y = min(max(y0 + ry - h, 0), a.height - 1);
				const GlobalIn p = in + (long long) y * a.in_stride + 3LL * x;
				short L, A = 0, B = 0;
				sq_to_labs<false>(s_blk, s_res, s_v2Y, p[0], p[1], p[2], L, A, B);
				s_L[ry * SQ_R + rx] = L;
			}
		}
		__syncthreads();
		// 2. horizontal pass on L (all rows of the region, the tile's columns)
		for (int idx = t; idx < rw * SQ_T; idx += SQ_NT) {
			const int ry = idx >> 6, cx = idx & 63;
			int sum = 0;
#pragma unroll
			for (int k = 0; k < 2 * SF_MAXHALF + 1; k++)
				sum += a.coef[k] * (int) s_L[ry * SQ_R + cx + k];
			s_h[ry * SQ_T + cx] = (short) sf_convi_fin(sum, a);
		}
		__syncthreads();
		// 3. vertical pass, the LUT, back to sRGB: 4 pixels per thread, three dword stores
		{
			const int y = y0 + row;
			if (y < a.height) {
				unsigned char o[12];
#pragma unroll
				for (int m = 0; m < 4; m++) {
					const int cx = 4 * quad + m;
					int sum = 0;
#pragma unroll
					for (int k = 0; k < 2 * SF_MAXHALF + 1; k++)
						sum += a.coef[k] * (int) s_h[(row + k) * SQ_T + cx];
					const int blur = sf_convi_fin(sum, a);
					const int v1 = s_L[(row + h) * SQ_R + cx + h];
					// sharpen.c:116-168: index (v1 & 0x7fff) - (blur & 0x7fff) + 32768 of the LUT
					const int d = (v1 & 0x7fff) - (blur & 0x7fff) + 32768 - q.lut_lo;
					int lv = d < 0 ? q.lut_below : q.lut_above;
					if ((unsigned int) d < (unsigned int) q.lut_n)
						lv = s_lut[d];
					const int sharp = min(max(v1 + lv, 0), 32767);
					const unsigned int ab = s_ab[row * SQ_T + cx];
					labs_to_srgb8(s_Y2v, sharp, (int) (short) (ab & 0xffffu), (int) ab >> 16, o[3 * m], o[3 * m + 1], o[3 * m + 2]);
				}
				const int x = x0 + 4 * quad;
				const GlobalOut dst = out + (long long) y * a.out_stride + 3LL * x;
				if (x + 4 <= a.width && !(((uintptr_t) dst) & 3)) {
					unsigned int __attribute__((address_space(1))) *d4 = (unsigned int __attribute__((address_space(1))) *) dst;
#pragma unroll
					for (int w = 0; w < 3; w++)
						d4[w] = (unsigned) o[4 * w] | ((unsigned) o[4 * w + 1] << 8) | ((unsigned) o[4 * w + 2] << 16) |
							((unsigned) o[4 * w + 3] << 24);
				}
				else {
					for (int m = 0; m < 12 && x + m / 3 < a.width; m++)
						dst[m] = o[m];
				}
			}
		}
	}
}

// n images of one geometry (one launch per SF_MAXB of them).  0 done, 1 not this kernel's case, -1 error
// Per device, once: does every colour come back from sRGB -> LabS -> sRGB (sharpen_identity_kernel)?  A failure
// to run the check counts as "no": the kernel that takes every pixel the whole way needs no such proof.
static bool sharpen_identity_proven(const ColourTables &tables)
{
	constexpr int MAXDEV = 64;
	static std::mutex mutex;
	static signed char state[MAXDEV]; // 0 unknown, 1 proven, -1 not
	const int dev = current_device();
	if (dev < 0 || dev >= MAXDEV)
		return false;
	std::lock_guard<std::mutex> lock(mutex);
	if (state[dev] == 0) {
		state[dev] = -1;
		unsigned int zero = 0, bad = 1;
		unsigned int *d_bad = (unsigned int *) upload(&zero, sizeof(zero));
		if (d_bad) {
			hipLaunchKernelGGL(sharpen_identity_kernel, dim3(65536), dim3(256), 0, stream(), tables, d_bad);
			if (hipGetLastError() == hipSuccess &&
				hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, stream()) == hipSuccess &&
				hipStreamSynchronize(stream()) == hipSuccess && bad == 0)
				state[dev] = 1;
			vips_hip_free(d_bad);
		}
		else
			vips_hip_error_clear();
	}
	return state[dev] == 1;
}

// sharpen_quad_u8_kernel's 106 KB of dynamic LDS need the opt-in, which is a per-device attribute of the function
static bool sharpen_quad_lds_allowed()
{
	constexpr int MAXDEV = 64;
	static std::mutex mutex;
	static signed char state[MAXDEV];
	const int dev = current_device();
	if (dev < 0 || dev >= MAXDEV)
		return false;
	std::lock_guard<std::mutex> lock(mutex);
	if (state[dev] == 0) {
		const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(sharpen_quad_u8_kernel),
			hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
		state[dev] = e == hipSuccess ? 1 : -1;
		if (e != hipSuccess)
			(void) hipGetLastError();
	}
	return state[dev] == 1;
}

int sharpen_fused_u8(const VipsHipRegion *const *ins, const VipsHipRegion *const *outs, int n_images,
	const int *to_steps, int n_to, const int *from_steps, int n_from, const int *coef, int n, int scale,
	const int *lut, const SharpenLutWindow *win)
{
	if (getenv("VIPS_HIP_NO_FUSED_SHARPEN") || n_images < 1)
		return 1;
	const VipsHipRegion *in = ins[0], *out = outs[0];
	for (int i = 0; i < n_images; i++) {
		const VipsHipRegion *ri = ins[i], *ro = outs[i];
		if (ri->format != VIPS_HIP_FORMAT_UCHAR || ro->format != VIPS_HIP_FORMAT_UCHAR || ri->bands != 3 ||
			ro->bands != 3)
			return 1;
		if (ri->left != 0 || ri->top != 0 || ro->left != 0 || ro->top != 0 || ri->width != ri->im_width ||
			ri->height != ri->im_height || ro->width != ri->width || ro->height != ri->height)
			return 1;
		if (ri->width != in->width || ri->height != in->height || ri->stride != in->stride ||
			ro->stride != out->stride)
			return 1;
	}
	if (n < 1 || n > 2 * SF_MAXHALF + 1 || !(n & 1) || scale <= 0)
		return 1;
	long long abs_sum = 0;
	for (int k = 0; k < n; k++)
		abs_sum += coef[k] < 0 ? -(long long) coef[k] : coef[k];
	if (abs_sum * 32768 + scale >= (1LL << 31)) // 32-bit sums
		return 1;
	// the kernel runs the two chains vips_sharpen uses on sRGB, spelled out
	static const int want_to[4] = { VIPS_HIP_COLOUR_sRGB2scRGB, VIPS_HIP_COLOUR_scRGB2XYZ, VIPS_HIP_COLOUR_XYZ2Lab,
		VIPS_HIP_COLOUR_Lab2LabS };
	static const int want_from[4] = { VIPS_HIP_COLOUR_LabS2Lab, VIPS_HIP_COLOUR_Lab2XYZ, VIPS_HIP_COLOUR_XYZ2scRGB,
		VIPS_HIP_COLOUR_scRGB2sRGB };
	if (n_to != 4 || n_from != 4 || memcmp(to_steps, want_to, sizeof(want_to)) ||
		memcmp(from_steps, want_from, sizeof(want_from)))
		return 1;
	SharpenFusedArgs a;
	RouteArgs to_labs;
	if (colour_route_prepare(to_steps, n_to, &to_labs))
		return -1;
	a.tables = to_labs.tables;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) out->stride;
	a.width = in->width;
	a.height = in->height;
	a.n = n;
	a.half = n / 2;
	for (int k = 0; k < 2 * SF_MAXHALF + 1; k++)
		a.coef[k] = k < n ? coef[k] : 0;
	a.scale = scale;
	a.rounding = scale / 2;
	a.magic = 0;
	a.shift = 0;
	if (scale > 1) {
		int l = 0;
		while ((1LL << l) < scale)
			l++;
		a.magic = (unsigned int) ((((1ULL << 32) * ((1ULL << l) - (unsigned long long) scale)) / (unsigned long long) scale) + 1);
		a.shift = l - 1;
	}
	a.lut = lut;
	// the blur's division as a 24-bit multiply-high: tried on every sum the mask can make (under a million)
	// (once per (scale, largest sum): the answer is kept)
	a.sh24 = -1;
	a.m24 = 0;
	{
		const long long n_max = abs_sum * 32767 + a.rounding;
		static std::mutex mutex;
		static std::map<std::pair<int, long long>, std::pair<int, unsigned int>> proven;
		std::lock_guard<std::mutex> lock(mutex);
		auto it = proven.find(std::make_pair(scale, n_max));
		if (it == proven.end()) {
			std::pair<int, unsigned int> answer(-1, 0u);
			int sh = 0;
			while (sh < 24 && (n_max << (sh + 1)) < (1LL << 24))
				sh++;
			const unsigned long long m = ((1ULL << (32 - sh)) + (unsigned long long) scale - 1) / (unsigned long long) scale;
			if (n_max < (1LL << 24) && (n_max << sh) < (1LL << 24) && m < (1ULL << 24)) {
				bool ok = true;
				for (long long v = 0; v <= n_max && ok; v++)
					ok = (((unsigned long long) (v << sh) * m) >> 32) == (unsigned long long) (v / scale);
				if (ok)
					answer = std::make_pair(sh, (unsigned int) m);
			}
			if (proven.size() > 64)
				proven.clear();
			it = proven.emplace(std::make_pair(scale, n_max), answer).first;
		}
		a.sh24 = it->second.first;
		a.m24 = it->second.second;
	}
	a.zero_lo = win ? win->zero_lo : 1;
	a.zero_hi = win ? win->zero_hi : 0;
	// every table in LDS (sharpen_quad_u8_kernel) when the LUT's window and this host's cbrtf allow it -- for large
	// images.  Measured (profiles/r05p_sharpen_quad.txt): 8192^2 of noise 1.08 -> 0.83 ms, but a batch of 1024^2
	// thumbnails on its 64-CU partition 0.033 -> 0.049 ms per image: a thumbnail's values are few and near each
	// other, the older kernel's table gathers hit its L1, and 106 KB of LDS per block leave that partition one block
	// of 16 waves per CU to hide behind.  $VIPS_HIP_SHARPEN_QUAD=0 / 1 forces one or the other.
	// the pixels the LUT leaves alone skip the way back (sharpen_fused_u8_kernel<*, true>) when the LUT has a zero
	// window at all and sRGB -> LabS -> sRGB is the identity with this device's tables.  $VIPS_HIP_SHARPEN_SKIP=0:
	// every pixel the whole way.
	const char *skip_env = getenv("VIPS_HIP_SHARPEN_SKIP");
	bool nonneg = true; // (a gaussian's integer mask: what lets the skip kernel divide without a sign)
	for (int k = 0; k < n; k++)
		nonneg = nonneg && coef[k] >= 0;
	const bool small = (long long) a.height * a.in_stride < (1LL << 31) && a.in_stride < (1LL << 24) && a.height < (1 << 24) &&
		a.in_stride >= 0;
	const bool skip = nonneg && small && a.sh24 >= 0 && a.zero_lo <= 0 && a.zero_hi >= 0 && !(skip_env && atoi(skip_env) == 0) &&
		sharpen_identity_proven(a.tables);
	a.defer = nullptr;
	a.defer_threshold = 0;
	a.defer_raw = 0;
	a.q_tiles_x = a.q_tiles_y = 0;
	const char *quad_env = getenv("VIPS_HIP_SHARPEN_QUAD");
	const bool want_quad = quad_env ? atoi(quad_env) != 0 : (long long) a.width * a.height >= 2048LL * 2048;
	// (the LDS opt-in is per DEVICE: asked for on every device this code reaches; a device that refuses it keeps
	// the kernel that needs none)
	if (win && win->lut_win && win->n <= SQ_MAXLUT && want_quad && !getenv("VIPS_HIP_NO_SHARPEN_QUAD") &&
		sharpen_quad_lds_allowed()) {
		const CbrtQuad *cq = cbrt_quad_tables();
		if (cq) {
			SharpenQuadArgs q;
			q.f = a;
			q.cq = *cq;
			q.lut_win = win->lut_win;
			q.lut_lo = win->lo;
			q.lut_n = win->n;
			q.lut_below = win->below;
			q.lut_above = win->above;
			q.tiles_x = (a.width + SQ_T - 1) / SQ_T;
			q.tiles_y = (a.height + SQ_T - 1) / SQ_T;
			const size_t lds = (size_t) (CBQ_BLOCKS * 4 + CBQ_RES_WORDS + 256 + 260) * 4 + (size_t) (SQ_MAXLUT + 8) * 2 +
				(size_t) SQ_R * SQ_R * 2 + (size_t) SQ_T * SQ_T * 4 + (size_t) SQ_R * SQ_T * 2;
			// Large images (round 6), ADAPTIVELY: what a photograph mostly is -- neighbouring pixels near each other,
			// the LUT's flat centre -- is what the skip kernel is fast at (8192^2 smooth: 0.79 -> ~0.3 ms), noise and
			// dense edges what this one is (0.83 against ~1.2).  So the skip kernel goes first and LEAVES the tiles
			// whose list is long (more than defer_threshold of a 64 x 32 tile's 2 048 pixels) on a device-side list;
			// this kernel then walks that list -- no host round trip, the count is read on the device.
			// $VIPS_HIP_SHARPEN_ADAPTIVE=0: this kernel alone, every tile.
			const char *ad = getenv("VIPS_HIP_SHARPEN_ADAPTIVE");
			const bool adaptive = skip && a.n <= 5 && a.height > 16 && !(ad && atoi(ad) == 0);
			q.defer = nullptr;
			for (int base = 0; base < n_images; base += SF_MAXB) {
				const int count = n_images - base < SF_MAXB ? n_images - base : SF_MAXB;
				SharpenFusedPtrs p;
				memset(&p, 0, sizeof(p));
				for (int i = 0; i < count; i++) {
					p.in[i] = (const unsigned char *) ins[base + i]->data;
					p.out[i] = (unsigned char *) outs[base + i]->data;
				}
				q.n_images = count;
				const int tiles = q.tiles_x * q.tiles_y * count;
				int *defer = nullptr;
				if (adaptive) {
					defer = (int *) vips_hip_malloc((size_t) (1 + 2 * tiles) * sizeof(int));
					if (!defer)
						return -1;
					if (hipMemsetAsync(defer, 0, (size_t) (1 + tiles) * sizeof(int), stream()) != hipSuccess) {
						vips_hip_free(defer);
						error("sharpen", "memset failed");
						return -1;
					}
					SharpenFusedArgs a1 = a;
					a1.defer = defer;
					a1.defer_threshold = getenv("VIPS_HIP_SHARPEN_DEFER") ? atoi(getenv("VIPS_HIP_SHARPEN_DEFER")) : 640;
					a1.defer_raw = getenv("VIPS_HIP_SHARPEN_DEFER_RAW") ? atoi(getenv("VIPS_HIP_SHARPEN_DEFER_RAW")) : 24; // (12 sends a fifth of a smooth image's tiles the slow way: profiles/r06n_sharpen_raw.txt)
					a1.q_tiles_x = q.tiles_x;
					a1.q_tiles_y = q.tiles_y;
					dim3 grid1((a.width + SF_TW - 1) / SF_TW, (a.height + 31) / 32, count);
					if (a1.defer_raw > 0) {
						Gate gate0("sharpen_survey");
						const int stx = (int) grid1.x, sty = (int) grid1.y;
						hipLaunchKernelGGL(sharpen_survey_kernel, dim3((stx * sty + 255) / 256, 1, count), dim3(256, 1, 1), 0, stream(), p,
							a.width, a.height, (long long) a.in_stride, a1.defer_raw, defer, q.tiles_x, q.tiles_y, stx, sty);
					}
					Gate gate1("sharpen_skip_u8");
					if (a.n <= 3)
						hipLaunchKernelGGL((sharpen_fused_u8_kernel<32, true, 3>), grid1, dim3(256, 1, 1), 0, stream(), p, a1);
					else
						hipLaunchKernelGGL((sharpen_fused_u8_kernel<32, true, 5>), grid1, dim3(256, 1, 1), 0, stream(), p, a1);
					if (hipGetLastError() != hipSuccess) {
						vips_hip_free(defer);
						error("sharpen", "kernel launch failed");
						return -1;
					}
				}
				q.defer = defer;
				const char *e = getenv("VIPS_HIP_SHARPEN_QUAD_GRID");
				int grid = e && atoi(e) > 0 ? atoi(e) : 256;
				grid = grid > tiles ? tiles : grid;
				{
					Gate gate("sharpen_quad_u8");
					hipLaunchKernelGGL(sharpen_quad_u8_kernel, dim3(grid), dim3(SQ_NT), lds, stream(), p, q);
				}
				const bool ok = hipGetLastError() == hipSuccess;
				if (defer)
					vips_hip_free(defer); // (reuse is ordered on this thread's stream)
				if (!ok) {
					error("sharpen", "kernel launch failed");
					return -1;
				}
			}
			return 0;
		}
		vips_hip_error_clear();
	}
	Gate gate(skip ? "sharpen_skip_u8" : "sharpen_fused_u8");
	for (int base = 0; base < n_images; base += SF_MAXB) {
		const int count = n_images - base < SF_MAXB ? n_images - base : SF_MAXB;
		SharpenFusedPtrs p;
		memset(&p, 0, sizeof(p));
		for (int i = 0; i < count; i++) {
			p.in[i] = (const unsigned char *) ins[base + i]->data;
			p.out[i] = (unsigned char *) outs[base + i]->data;
		}
		// 32-row tiles: the halo ring and the block's table loads are shared by twice the pixels
		// (2 % faster than 16-row tiles in the C4 batch, 64-row tiles slower again);
		// $VIPS_HIP_SHARPEN_TH=16 for the other
		const int th = getenv("VIPS_HIP_SHARPEN_TH") ? atoi(getenv("VIPS_HIP_SHARPEN_TH")) : 32;
		if (th != 16 && a.height > 16) {
			dim3 grid((a.width + SF_TW - 1) / SF_TW, (a.height + 31) / 32, count);
			if (skip && a.n <= 3)
				hipLaunchKernelGGL((sharpen_fused_u8_kernel<32, true, 3>), grid, dim3(256, 1, 1), 0, stream(), p, a);
			else if (skip)
				hipLaunchKernelGGL((sharpen_fused_u8_kernel<32, true, 5>), grid, dim3(256, 1, 1), 0, stream(), p, a);
			else
				hipLaunchKernelGGL((sharpen_fused_u8_kernel<32, false>), grid, dim3(256, 1, 1), 0, stream(), p, a);
		}
		else {
			dim3 grid((a.width + SF_TW - 1) / SF_TW, (a.height + 15) / 16, count);
			if (skip && a.n <= 3)
				hipLaunchKernelGGL((sharpen_fused_u8_kernel<16, true, 3>), grid, dim3(256, 1, 1), 0, stream(), p, a);
			else if (skip)
				hipLaunchKernelGGL((sharpen_fused_u8_kernel<16, true, 5>), grid, dim3(256, 1, 1), 0, stream(), p, a);
			else
				hipLaunchKernelGGL((sharpen_fused_u8_kernel<16, false>), grid, dim3(256, 1, 1), 0, stream(), p, a);
		}
		VH_CHECK(hipGetLastError());
	}
	return 0;
}

} // namespace vh

using namespace vh;

extern "C" {

int vips_hip_sharpen_gen(const int *lut_device, const VipsHipRegion *in,
	const VipsHipRegion *blurred_l, const VipsHipRegion *out)
{
	const char *domain = "sharpen";
	if (ensure_init())
		return -1;
	if (check_region(domain, in) || check_region(domain, blurred_l) || check_region(domain, out))
		return -1;
	if (in->format != VIPS_HIP_FORMAT_SHORT || out->format != VIPS_HIP_FORMAT_SHORT ||
		blurred_l->format != VIPS_HIP_FORMAT_SHORT || blurred_l->bands != 1 ||
		in->bands != out->bands) {
		error(domain, "need LabS short images (and a 1-band blurred L)");
		return -1;
	}
	if (!lut_device) {
		error(domain, "null lut");
		return -1;
	}
	for (const VipsHipRegion *r : { in, blurred_l })
		if (out->left < r->left || out->top < r->top || out->left + out->width > r->left + r->width ||
			out->top + out->height > r->top + r->height) {
			error(domain, "input region too small");
			return -1;
		}
	SharpenArgs a;
	a.in = (const unsigned char *) in->data + (size_t) (out->top - in->top) * in->stride +
		(size_t) (out->left - in->left) * in->bands * 2;
	a.blur = (const unsigned char *) blurred_l->data +
		(size_t) (out->top - blurred_l->top) * blurred_l->stride +
		(size_t) (out->left - blurred_l->left) * 2;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.blur_stride = (long long) blurred_l->stride;
	a.out_stride = (long long) out->stride;
	a.width = out->width;
	a.height = out->height;
	a.bands = in->bands;
	a.lut = lut_device;
	dim3 block(256, 1, 1);
	dim3 grid((a.width + 255) / 256, rows_grid((a.width + 255) / 256, a.height), 1);
	Gate gate("sharpen");
	hipLaunchKernelGGL(sharpen_kernel, grid, block, 0, stream(), a);
	VH_CHECK(hipGetLastError());
	return 0;
}

} // extern "C"
