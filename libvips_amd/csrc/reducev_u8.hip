// uchar fast paths for gfx950, one axis -- see reduce_u8.h.  The vertical kernels never look across a scanline, so
// they take any band count: reducev_u8_mfma (an integer 8 with one phase, on the matrix cores), reducev_u8_kernel
// (any geometry, row pairs on the vector ALU) and shrinkv_u8_kernel.
#include "reduce_u8_host.h"

#include <cstdlib>

namespace vh {

// ------------------------------------------------- vertical uchar fast kernels
//
// reducev and shrinkv never look across a scanline, so a uchar image of any band count
// is a byte array per row: each thread owns DW consecutive dwords of the row (16 bytes
// when the geometry allows -> 1 KiB contiguous per wave per row) and walks the taps.

struct VerticalArgs {
	const unsigned char *in; // already offset to the first column of the rect
	unsigned char *out;
	long long in_stride, out_stride;
	int in_top, im_height;
	int out_top, out_height;
	int ndw; // dwords per row
};

// reducev.cpp:418-459 / reducev_hwy.cpp:94-268: sum_i k[i] * in[x + i * lskip], +2048, >>12,
// saturate.  Rows are taken in pairs so one v_dot2 does two taps of one byte lane.
template <int DW>
__global__ void __launch_bounds__(256)
reducev_u8_kernel(VerticalArgs a, int n_point, const ReducePos *__restrict__ pos,
	const short *__restrict__ table, int gx, int band)
{
	// Neighbouring output rows share most of their input rows, and an L2 is per XCD: block b
	// runs on XCD b % 8, so give each XCD one contiguous band of output rows (a row-major
	// grid would make all 8 L2s fetch every input row).
	const int local = blockIdx.x / 8;
	const int yb = local / gx;
	const int t = (local - yb * gx) * blockDim.x + threadIdx.x;
	const int y = (blockIdx.x % 8) * band + yb;
	if (t * DW >= a.ndw || y >= a.out_height)
		return;
	constexpr int BATCH = 8; // rows fetched before any is used: 8 loads in flight per lane
	{
		const ReducePos p = pos[y];
		const short *c = table + (size_t) p.phase * n_point;
		int acc[DW][4];
#pragma unroll
		for (int w = 0; w < DW; w++)
#pragma unroll
			for (int k = 0; k < 4; k++)
				acc[w][k] = 0;
		for (int i0 = 0; i0 < n_point; i0 += BATCH) {
			unsigned int v[BATCH][DW];
#pragma unroll
			for (int j = 0; j < BATCH; j++) {
				// past the last tap: re-fetch the last row (the window need not hold more), coefficient 0
				const int r = min(max(p.first + min(i0 + j, n_point - 1), 0), a.im_height - 1) - a.in_top;
				const unsigned int *pr = (const unsigned int *) (a.in + r * a.in_stride) + t * DW;
				if (DW == 4) {
					const uint4 x = *reinterpret_cast<const uint4 *>(pr);
					v[j][0] = x.x, v[j][1 % DW] = x.y, v[j][2 % DW] = x.z, v[j][3 % DW] = x.w;
				}
				else {
#pragma unroll
					for (int w = 0; w < DW; w++)
						v[j][w] = pr[w];
				}
			}
#pragma unroll
			for (int j = 0; j < BATCH; j += 2) {
				const int i = i0 + j;
				const unsigned int lo = i < n_point ? (unsigned short) c[i] : 0u;
				const unsigned int hi = i + 1 < n_point ? (unsigned short) c[i + 1] : 0u;
				const unsigned int coef = lo | (hi << 16);
#pragma unroll
				for (int w = 0; w < DW; w++)
#pragma unroll
					for (int k = 0; k < 4; k++) {
						const unsigned int pair = __builtin_amdgcn_perm(v[j + 1][w], v[j][w],
							0x0c000c00u | (unsigned) k | ((4u + k) << 16));
						acc[w][k] = dot2(pair, coef, acc[w][k]);
					}
			}
		}
		unsigned int *dst = (unsigned int *) (a.out + (long long) y * a.out_stride) + t * DW;
		unsigned int o[DW];
#pragma unroll
		for (int w = 0; w < DW; w++)
			o[w] = (unsigned) fin_u8(acc[w][0]) | ((unsigned) fin_u8(acc[w][1]) << 8) |
				((unsigned) fin_u8(acc[w][2]) << 16) | ((unsigned) fin_u8(acc[w][3]) << 24);
		if (DW == 4)
			*reinterpret_cast<uint4 *>(dst) = make_uint4(o[0], o[1 % DW], o[2 % DW], o[3 % DW]);
		else {
#pragma unroll
			for (int w = 0; w < DW; w++)
				dst[w] = o[w];
		}
	}
}

// shrinkv.c:158-165,218-228 / shrinkv_hwy.cpp:90-203: column sums of vshrink rows, then
// ((sum + vshrink/2) * (2^32 / (256 * vshrink))) >> 24 in unsigned 32-bit arithmetic.
constexpr int SHRINKV_MAXB = 64; // images per launch (blockIdx.z)

// the images of a launch, read where they lie in the kernarg segment
struct ShrinkvPtrs {
	const unsigned char *in[SHRINKV_MAXB]; // already offset to the first column of the rect
	unsigned char *out[SHRINKV_MAXB];
};

template <int DW>
__global__ void __launch_bounds__(256)
shrinkv_u8_kernel(ShrinkvPtrs ptrs_by_value, VerticalArgs a, int vshrink, unsigned int multiplier)
{
	(void) ptrs_by_value;
	typedef const unsigned long long __attribute__((address_space(4))) *KernargPtrs;
	const KernargPtrs kp = (KernargPtrs) __builtin_amdgcn_kernarg_segment_ptr();
	// (pointers made from integers are generic to the compiler: say they are global)
	typedef const unsigned char __attribute__((address_space(1))) *GlobalIn;
	typedef unsigned char __attribute__((address_space(1))) *GlobalOut;
	const GlobalIn in = (GlobalIn) kp[blockIdx.z];
	const GlobalOut out = (GlobalOut) kp[SHRINKV_MAXB + blockIdx.z];
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t * DW >= a.ndw)
		return;
	const unsigned int amend = vshrink / 2;
	for (int y = blockIdx.y; y < a.out_height; y += gridDim.y) {
		const int y0 = (a.out_top + y) * vshrink;
		// even / odd bytes as two u16 lanes each: packed adds, no carries for vshrink <= 256
		unsigned int even[DW], odd[DW];
#pragma unroll
		for (int w = 0; w < DW; w++)
			even[w] = odd[w] = 0;
		for (int i = 0; i < vshrink; i++) {
			const int row = min(y0 + i, a.im_height - 1) - a.in_top;
			typedef unsigned int sv_uint4 __attribute__((ext_vector_type(4)));
			const unsigned int __attribute__((address_space(1))) *p =
				(const unsigned int __attribute__((address_space(1))) *) (in + row * a.in_stride) + t * DW;
			unsigned int v[DW];
			if (DW == 4) {
				const sv_uint4 x = *(const sv_uint4 __attribute__((address_space(1))) *) p;
				v[0] = x.x, v[1 % DW] = x.y, v[2 % DW] = x.z, v[3 % DW] = x.w;
			}
			else {
#pragma unroll
				for (int w = 0; w < DW; w++)
					v[w] = p[w];
			}
#pragma unroll
			for (int w = 0; w < DW; w++) {
				even[w] += v[w] & 0x00ff00ffu;
				odd[w] += (v[w] >> 8) & 0x00ff00ffu;
			}
		}
		unsigned int __attribute__((address_space(1))) *dst =
			(unsigned int __attribute__((address_space(1))) *) (out + (long long) y * a.out_stride) + t * DW;
		unsigned int o[DW];
#pragma unroll
		for (int w = 0; w < DW; w++) {
			const unsigned int b0 = (((even[w] & 0xffffu) + amend) * multiplier) >> 24;
			const unsigned int b2 = (((even[w] >> 16) + amend) * multiplier) >> 24;
			const unsigned int b1 = (((odd[w] & 0xffffu) + amend) * multiplier) >> 24;
			const unsigned int b3 = (((odd[w] >> 16) + amend) * multiplier) >> 24;
			o[w] = (b0 & 0xffu) | ((b1 & 0xffu) << 8) | ((b2 & 0xffu) << 16) | (b3 << 24);
		}
		if (DW == 4) {
			typedef unsigned int sv_uint4 __attribute__((ext_vector_type(4)));
			const sv_uint4 ov = { o[0], o[1 % DW], o[2 % DW], o[3 % DW] };
			*(sv_uint4 __attribute__((address_space(1))) *) dst = ov;
		}
		else {
#pragma unroll
			for (int w = 0; w < DW; w++)
				dst[w] = o[w];
		}
	}
}

// Common geometry of the vertical fast paths: the rect's rows as dword arrays.
static bool vertical_args(const VipsHipRegion *in, const VipsHipRegion *out, VerticalArgs *a, int *dw)
{
	const int bands = in->bands;
	const long long nbytes = (long long) out->width * bands;
	const unsigned char *src = (const unsigned char *) in->data + (size_t) (out->left - in->left) * bands;
	if (nbytes & 3)
		return false;
	if (((uintptr_t) src & 3) || (in->stride & 3) || ((uintptr_t) out->data & 3) || (out->stride & 3))
		return false;
	a->in = src;
	a->out = (unsigned char *) out->data;
	a->in_stride = (long long) in->stride;
	a->out_stride = (long long) out->stride;
	a->in_top = in->top;
	a->im_height = in->im_height;
	a->out_top = out->top;
	a->out_height = out->height;
	a->ndw = (int) (nbytes >> 2);
	const bool wide = !(nbytes & 15) && !((uintptr_t) src & 15) && !(in->stride & 15) &&
		!((uintptr_t) out->data & 15) && !(out->stride & 15);
	*dw = wide ? 4 : 1;
	return true;
}

// ------------------------------------------------ vertical-only pass on the matrix cores
//
// reducev_u8_mfma<D>: vips_reducev by an integer 8 with one coefficient phase on a uchar image
// of ANY band count.  A scanline is a byte array to a vertical filter, so this is the fused
// kernel's vertical pass alone: a lane owns 8 consecutive bytes of the row, walks down the
// rows in groups of 8 with the same rotating MFMA accumulators, and each group retires one
// output row straight to memory (8 bytes per lane, a wave writes 512 contiguous bytes).  Every
// input byte is read once (the row-pair dot2 kernel re-reads each row n / 8 times through L2).
struct VStreamArgs {
	const unsigned char *in;  // first byte of the columns of the rect, row in_top of the image
	unsigned char *out;
	long long in_stride, out_stride;
	int in_top, im_height;
	int out_height;          // rows of the rect
	int fy0;                 // first tap (input row) of output row 0 of the rect
	int row_u2;              // 8-byte columns per row
	int oht, tiles_x, tiles; // tile = 256 columns x oht output rows
	int alternate;           // every other row of tiles is walked bottom-up
};

template <int D>
struct VStreamStep {
	static constexpr int S = 8;

	template <int I0, int N>
	static __device__ __forceinline__ void load_rows(const VStreamArgs &a, uint2 (&px)[S], int first_row, int dir,
		unsigned int coff)
	{
		const unsigned int stride32 = (unsigned int) a.in_stride;
#pragma unroll
		for (int i = I0; i < I0 + N; i++) {
			const int row = min(max(first_row + dir * i, 0), a.im_height - 1) - a.in_top;
			px[i] = *reinterpret_cast<const uint2 *>(a.in + (size_t) ((unsigned int) row * stride32 + coff));
		}
	}

	template <int ROT, int Q>
	static __device__ __forceinline__ void quad(const VStreamArgs &a, uint2 (&px)[S], float4v (&acc)[8][2],
		const half4v *lane_a, bool more, int next_row, int dir, unsigned int coff)
	{
		const half4v a0 = lane_a[((ROT * 2 + Q) * 2 + 0) * 4];
		const half4v a1 = lane_a[((ROT * 2 + Q) * 2 + 1) * 4];
#pragma unroll
		for (int p = 0; p < 2; p++) {
			const unsigned int r0 = p ? px[4 * Q + 0].y : px[4 * Q + 0].x;
			const unsigned int r1 = p ? px[4 * Q + 1].y : px[4 * Q + 1].x;
			const unsigned int r2 = p ? px[4 * Q + 2].y : px[4 * Q + 2].x;
			const unsigned int r3 = p ? px[4 * Q + 3].y : px[4 * Q + 3].x;
			half4v b[4];
			b[0] = make_b<0>(r0, r1, r2, r3);
			b[1] = make_b<1>(r0, r1, r2, r3);
			b[2] = make_b<2>(r0, r1, r2, r3);
			b[3] = make_b<3>(r0, r1, r2, r3);
			if (p == 1 && more)
				load_rows<4 * Q, 4>(a, px, next_row, dir, coff);
#pragma unroll
			for (int c = 0; c < 4; c++) {
				acc[p * 4 + c][0] = __builtin_amdgcn_mfma_f32_4x4x4f16(a0, b[c], acc[p * 4 + c][0], 0, 0, 0);
				acc[p * 4 + c][1] = __builtin_amdgcn_mfma_f32_4x4x4f16(a1, b[c], acc[p * 4 + c][1], 0, 0, 0);
			}
		}
	}

	template <int ROT>
	static __device__ __forceinline__ void retire(float4v (&acc)[8][2], unsigned char *dst, bool store)
	{
		constexpr int SLOT = (ROT - (D - 1) + 2 * MFMA_SLOTS) % MFMA_SLOTS;
		constexpr int H = SLOT >> 2, I = SLOT & 3;
		if (store) {
			uint2 v;
			v.x = fin_pack(acc[3][H][I], 3,
				fin_pack(acc[2][H][I], 2, fin_pack(acc[1][H][I], 1, fin_pack(acc[0][H][I], 0, 0))));
			v.y = fin_pack(acc[7][H][I], 3,
				fin_pack(acc[6][H][I], 2, fin_pack(acc[5][H][I], 1, fin_pack(acc[4][H][I], 0, 0))));
			*reinterpret_cast<uint2 *>(dst) = v;
		}
#pragma unroll
		for (int o = 0; o < 8; o++)
			acc[o][H][I] = 0.0f;
	}

	// NB = prefetch depth: group g lives in ring buffer g mod NB (NB divides 8) and each of its quads is refilled
	// with group g + NB as soon as it has been consumed
	template <int ROT, int NB>
	static __device__ __forceinline__ void batch(const VStreamArgs &a, uint2 (&px)[NB][S], int g0, int ngroups,
		float4v (&acc)[8][2], const half4v *lane_a, int row0, int dir, unsigned int coff, unsigned char *out_col,
		int oh, bool active)
	{
		if constexpr (ROT < MFMA_SLOTS) {
			const int g = g0 + ROT;
			if (g < ngroups) {
				const bool more = g + NB < ngroups;
				const int next_row = row0 + dir * S * (g + NB);
				quad<ROT, 0>(a, px[ROT % NB], acc, lane_a, more, next_row, dir, coff);
				quad<ROT, 1>(a, px[ROT % NB], acc, lane_a, more, next_row, dir, coff);
				const int j = g - (D - 1); // row of the (possibly flipped) tile
				retire<ROT>(acc, out_col + (long long) (dir < 0 ? oh - 1 - j : j) * a.out_stride,
					active && j >= 0 && j < oh);
			}
			batch<ROT + 1, NB>(a, px, g0, ngroups, acc, lane_a, row0, dir, coff, out_col, oh, active);
		}
	}
};

template <int D, int NB, int OCC>
__global__ void __launch_bounds__(FUSED_THREADS, OCC)
reducev_u8_mfma(VStreamArgs a, const MfmaTables *__restrict__ tables)
{
	constexpr int S = 8;
	typedef VStreamStep<D> Step;
	__shared__ __attribute__((aligned(16))) half4v lds_a[MFMA_TABLE_ENTRIES];

	// each XCD takes a contiguous range of tiles (row-major: a tile row shares input rows)
	const int per_xcd = gridDim.x / 8;
	const int tile = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
	if (tile >= a.tiles)
		return;
	const int t = threadIdx.x;
	const int by = tile / a.tiles_x;
	const int bx = tile - by * a.tiles_x;
	const int y0 = by * a.oht;
	const int oh = min(a.oht, a.out_height - y0);
	const int col = bx * FUSED_THREADS + t;
	const bool active = col < a.row_u2;
	const unsigned int coff = 8u * (unsigned int) min(col, a.row_u2 - 1);
	// Every other row of tiles is walked bottom-up (the flipped problem: rows counted from the last one, taps
	// reversed -- tables->a[1], as in the fused kernel, reduce_fused_u8.hip): a tile and the one below it share 8 (D - 1) input
	// rows, which both now read at about the same time -- the second read is an L2 hit.  With every tile walking
	// down they were read a whole kernel apart: 263 MB fetched for an image of 201 (profiles/r05l_ops_traffic.txt).
	const bool flip = a.alternate && (by & 1);
	const int dir = flip ? -1 : 1;
	const int row0 = flip ? a.fy0 + S * (y0 + oh - 1) + S * D - 1 : a.fy0 + S * y0;

	if (t < MFMA_TABLE_ENTRIES)
		reinterpret_cast<uint2 *>(lds_a)[t] = reinterpret_cast<const uint2 *>(tables->a[flip ? 1 : 0])[t];
	const half4v *lane_a = lds_a + (t & 3);

	float4v acc[8][2];
#pragma unroll
	for (int o = 0; o < 8; o++)
#pragma unroll
		for (int h = 0; h < 2; h++)
			acc[o][h] = (float4v){ 0.0f, 0.0f, 0.0f, 0.0f };

	const int ngroups = oh + D - 1;
	uint2 px[NB][S];
#pragma unroll
	for (int b = 0; b < NB; b++)
		if (b < ngroups)
			Step::template load_rows<0, S>(a, px[b], row0 + dir * S * b, dir, coff);
	__syncthreads();

	unsigned char *out_col = a.out + (long long) y0 * a.out_stride + coff;
	for (int g0 = 0; g0 < ngroups; g0 += MFMA_SLOTS) {
		Step::template batch<0, NB>(a, px, g0, ngroups, acc, lane_a, row0, dir, coff, out_col, oh, active);
	}
}

// The matrix-core streaming kernel: integer-8 shrink, one phase, rows of whole 8-byte columns.
static int reducev_stream_try(const _VipsHipReduce *rc, const VipsHipRegion *in, const VipsHipRegion *out, int tile)
{
	if (getenv("VIPS_HIP_NO_MFMA"))
		return 0;
	_VipsHipReduce *r = const_cast<_VipsHipReduce *>(rc);
	const long long nbytes = (long long) out->width * in->bands;
	const unsigned char *src = (const unsigned char *) in->data + (size_t) (out->left - in->left) * in->bands;
	if ((nbytes & 7) || ((uintptr_t) src & 7) || (in->stride & 7) || ((uintptr_t) out->data & 7) ||
		(out->stride & 7))
		return 0;
	if (!(in->stride > 0 && (long long) in->stride * in->height < (1LL << 31)))
		return 0;
	std::vector<ReducePos> pv;
	reduce_positions(r, out->top, out->height, tile, pv);
	int fy0, sy, phase;
	if (!positions_regular(pv, &fy0, &sy, &phase) || (out->height > 1 && sy != 8))
		return 0;
	const int n = effective_taps(r, phase);
	const int D = (n + 7) / 8;
	if (D != 6 && D != 7)
		return 0;
	std::vector<int> taps;
	if (!mfma_taps(r, phase, D, taps))
		return 0;
	const MfmaTables *d_tables = mfma_tables_cached(r, std::make_tuple(-4, phase, 8 * D), taps, taps, D);
	if (!d_tables)
		return -1;
	VStreamArgs a;
	a.in = src;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) out->stride;
	a.in_top = in->top;
	a.im_height = in->im_height;
	a.out_height = out->height;
	a.fy0 = fy0;
	a.row_u2 = (int) (nbytes >> 3);
	a.tiles_x = (a.row_u2 + FUSED_THREADS - 1) / FUSED_THREADS;
	// two residency rounds of tiles (no LDS staging here, so several rounds cost nothing)
	int rows_of_tiles = 2048 / a.tiles_x;
	if (rows_of_tiles < 1)
		rows_of_tiles = 1;
	int oht = (out->height + rows_of_tiles - 1) / rows_of_tiles;
	// (a tile re-reads 8 (D - 1) rows of the one above: 32 output rows a tile where that still leaves 1.5 tiles a
	// CU -- 8192 x 8192 x 3 by 8: 0.0385 -> 0.0361 ms, profiles/r05o_reducev8_oht.txt -- else 16)
	if (oht < 32)
		oht = a.tiles_x * ((out->height + 31) / 32) >= 384 ? 32 : oht < 16 ? 16 : oht;
	if (const char *e = getenv("VIPS_HIP_REDUCEV8_OHT"))
		oht = atoi(e) > 0 ? atoi(e) : oht;
	a.oht = oht;
	a.alternate = !getenv("VIPS_HIP_BAND_NO_ALTERNATE");
	const int tiles_y = (out->height + oht - 1) / oht;
	a.tiles = a.tiles_x * tiles_y;
	const int grid = (a.tiles + 7) / 8 * 8;
	Gate gate("reducev_u8_mfma");
	// at most a tile a CU (images of a few tens of MB): four row groups in flight a lane, two blocks a CU's worth of
	// registers -- 4096 x 4096 x 3: 0.0166 -> 0.0129 ms; from 1.5 tiles a CU on it changes nothing
	// (profiles/r06f_reducev_nb.txt)
	const bool deep = getenv("VIPS_HIP_REDUCEV8_NB") ? atoi(getenv("VIPS_HIP_REDUCEV8_NB")) == 4 : a.tiles <= 256;
	if (D == 6 && deep)
		hipLaunchKernelGGL((reducev_u8_mfma<6, 4, 2>), dim3(grid), dim3(FUSED_THREADS), 0, stream(), a, d_tables);
	else if (D == 6)
		hipLaunchKernelGGL((reducev_u8_mfma<6, 1, 4>), dim3(grid), dim3(FUSED_THREADS), 0, stream(), a, d_tables);
	else if (deep)
		hipLaunchKernelGGL((reducev_u8_mfma<7, 4, 2>), dim3(grid), dim3(FUSED_THREADS), 0, stream(), a, d_tables);
	else
		hipLaunchKernelGGL((reducev_u8_mfma<7, 1, 4>), dim3(grid), dim3(FUSED_THREADS), 0, stream(), a, d_tables);
	if (hipGetLastError() != hipSuccess) {
		error("reducev", "kernel launch failed");
		return -1;
	}
	return 1;
}

int reducev_u8_try(const _VipsHipReduce *r, const VipsHipRegion *in, const VipsHipRegion *out,
	const ReducePos *pos, const short *table, int tile)
{
	{
		const int done = reducev_stream_try(r, in, out, tile);
		if (done != 0)
			return done;
	}
	{
		// a coefficient row per output row: the banded matrix on the matrix cores (reduce_band.hip)
		const int done = reducev_band_try(const_cast<_VipsHipReduce *>(r), in, out, tile);
		if (done != 0)
			return done;
	}
	{
		// ... or stream down the rows once on the vector ALU (resample16.hip)
		const int done = reducev8_stream_try(const_cast<_VipsHipReduce *>(r), in, out, tile);
		if (done != 0)
			return done;
	}
	VerticalArgs a;
	int dw;
	if (!vertical_args(in, out, &a, &dw))
		return 0;
	const int threads = (a.ndw + dw - 1) / dw;
	dim3 block(256, 1, 1);
	const int gx = (threads + 255) / 256;
	const int band = (out->height + 7) / 8;
	if ((long long) gx * band * 8 > 0x7fffffffLL)
		return 0;
	dim3 grid(gx * band * 8, 1, 1);
	Gate gate("reducev_u8");
	if (dw == 4)
		hipLaunchKernelGGL(reducev_u8_kernel<4>, grid, block, 0, stream(), a, r->n_point, pos, table, gx,
			band);
	else
		hipLaunchKernelGGL(reducev_u8_kernel<1>, grid, block, 0, stream(), a, r->n_point, pos, table, gx,
			band);
	if (hipGetLastError() != hipSuccess) {
		error("reducev", "kernel launch failed");
		return -1;
	}
	return 1;
}

// vips_shrinkv on n uchar rects of one geometry: one launch per SHRINKV_MAXB of them
int shrinkv_u8_batch_try(int vshrink, const VipsHipRegion *const *in, const VipsHipRegion *const *out, int n)
{
	if (n < 1 || vshrink > 256)
		return 0;
	VerticalArgs a;
	int dw;
	if (!vertical_args(in[0], out[0], &a, &dw))
		return 0;
	std::vector<VerticalArgs> each(n);
	for (int i = 0; i < n; i++) {
		int dwi;
		if (!vertical_args(in[i], out[i], &each[i], &dwi))
			return 0;
		const VerticalArgs &b = each[i];
		if (b.in_stride != a.in_stride || b.out_stride != a.out_stride || b.in_top != a.in_top ||
			b.im_height != a.im_height || b.out_top != a.out_top || b.out_height != a.out_height || b.ndw != a.ndw)
			return 0;
		dw = dwi < dw ? dwi : dw;
	}
	const unsigned int multiplier = (unsigned int) ((1LL << 32) / ((1 << 8) * (long long) vshrink));
	const int threads = (a.ndw + dw - 1) / dw;
	dim3 block(256, 1, 1);
	Gate gate("shrinkv_u8");
	for (int base = 0; base < n; base += SHRINKV_MAXB) {
		const int count = n - base < SHRINKV_MAXB ? n - base : SHRINKV_MAXB;
		ShrinkvPtrs p;
		memset(&p, 0, sizeof(p));
		for (int i = 0; i < count; i++) {
			p.in[i] = each[base + i].in;
			p.out[i] = each[base + i].out;
		}
		dim3 grid((threads + 255) / 256, a.out_height < 32768 ? a.out_height : 32768, count);
		if (dw == 4)
			hipLaunchKernelGGL(shrinkv_u8_kernel<4>, grid, block, 0, stream(), p, a, vshrink, multiplier);
		else
			hipLaunchKernelGGL(shrinkv_u8_kernel<1>, grid, block, 0, stream(), p, a, vshrink, multiplier);
		if (hipGetLastError() != hipSuccess) {
			error("shrinkv", "kernel launch failed");
			return -1;
		}
	}
	return 1;
}

int shrinkv_u8_try(int vshrink, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return shrinkv_u8_batch_try(vshrink, &in, &out, 1);
}

} // namespace vh
