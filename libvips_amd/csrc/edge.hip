// vips_sobel / vips_scharr / vips_prewitt (convolution/edge.c) and vips_compass (convolution/compass.c) on the device
// (gfx950).
//
//   edge_u8        The uchar path of the reference (vips_edge_build_uchar, edge.c:112-153) in ONE pass: two integer
//                  convolutions -- the 3 x 3 mask and its rot90, scale 2, offset 128 -- each rounded, offset and
//                  CLIPPED to 0 .. 255 exactly as vips_convi_gen does it (convi.c:698-716: the clip is observable,
//                  a conv of -300 and one of -128 both store 0), then vips_edge_uchar_gen (edge.c:96-104):
//                  |2 (c1 - 128)| + |2 (c2 - 128)| saturated at 255.  A block of 256 threads makes EDGE_TW = 1024
//                  elements x EDGE_TH = 16 rows from a halo tile in LDS (nbhd_tile.h), any band count.  A lane owns
//                  one DWORD of a row -- four elements -- so a mask position is a byte-shifted read of an LDS row:
//                  two aligned dwords and a funnel shift by a wave-uniform amount.  Both masks travel in the kernel
//                  arguments and are indexed by constants only (they live in scalar registers; a position where
//                  both are zero costs nothing).  The three LDS rows a mask column touches are read once a row of
//                  output: 9 shifted dwords feed 8 sums.
//   edge_combine   The per-element tail of the general tier: the two convolutions come from the conv kernels (conv.hip,
//                  each mask run as its OWN mask: the float conv adds a mask's non-zero elements in raster order,
//                  and rot90 changes that order), this kernel makes the output from them.
//                    float: vips_edge_build_float, edge.c:157-183 -- x * x and y * y rounded to float
//                           (vips_multiply), their float sum (vips_add), pow_const1(0.5) = 0 for 0 and sqrt in double
//                           stored as float otherwise (math2.c:147-162), vips_cast to uchar: clip as double,
//                           truncate (cast.c:231-238).  No fused multiply-add.
//                    uchar: vips_edge_uchar_gen on two uchar convolutions (the tail of edge_u8, for the cases the
//                           fused kernel leaves: the Highway arithmetic of convi, very wide pels).
//   compass_u8     vips_compass of a uchar image with precision integer and a 3 x 3 mask: up to eight rotated masks
//                  over edge_u8's tile, max / min / sum of the clipped convolutions, one read and one write.
//   canny_polar_thin  vips_canny behind its blur: the 2 x 2 gradient pair, the (G, theta) image and the thinning in one
//                  kernel, a uchar and a float instantiation; the float one counts the pels whose theta sits within
//                  4 ulp of atan2 of a float rounding boundary (vips_hip_canny_marginal).
//   compass_combine  The general tier's tail for vips_compass: abs, then max / min / sum over the convolutions of the
//                  distinct masks, in every format.
#include "nbhd_tile.h"

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>

namespace vh {

constexpr int EDGE_THREADS = 256;
constexpr int EDGE_TW = 4 * EDGE_THREADS; // elements = bytes
constexpr int EDGE_TH = 16;               // rows
constexpr int EDGE_COMBINE_ROWS = 65535;   // the most rows the combining kernels have in flight (grid.y)
constexpr int EDGE_LDS_MAX = 64 * 1024;

struct EdgeArgs {
	NbArgs nb;
	int c1[9], c2[9]; // the mask and its rot90, raster order
};

// vips_convi_gen's tail for uchar with scale 2 (rounding 1) and offset 128: C division truncates toward zero
VH_DEV int edge_conv_clip(int sum)
{
	const int v = (sum + 1) / 2 + 128;
	return v < 0 ? 0 : v > 255 ? 255 : v;
}

// vips_edge_uchar_gen, edge.c:96-104
VH_DEV unsigned int edge_uchar(int p1, int p2)
{
	int v1 = 2 * (p1 - 128), v2 = 2 * (p2 - 128);
	v1 = v1 < 0 ? -v1 : v1;
	v2 = v2 < 0 ? -v2 : v2;
	const int v = v1 + v2;
	return (unsigned int) (v > 255 ? 255 : v);
}

__global__ void __launch_bounds__(EDGE_THREADS)
edge_u8_kernel(EdgeArgs m)
{
	VH_DYNAMIC_LDS(unsigned int, lds);
	const NbArgs &a = m.nb;

	const int out_e0 = a.out_left * a.bands + (int) blockIdx.x * EDGE_TW;
	const int y0 = (int) blockIdx.y * EDGE_TH;
	const int s = out_e0 - a.bands; // the left halo: one pel
	const int s_al = s & ~3;
	const int lead = s - s_al;
	nb_stage<1, false>(a, lds, s_al, a.out_top + y0 - 1, EDGE_TH + 2, EDGE_THREADS);
	barrier();

	const int t = tid();
	const int e = (int) blockIdx.x * EDGE_TW + 4 * t; // the lane's first element, of the output rect's row
	const int out_elems = a.out_width * a.bands;
	const int row_dwords = a.lds_row >> 2;
	for (int ty = 0; ty < EDGE_TH; ty++) {
		if (y0 + ty >= a.out_height)
			break;
		int s1[4] = { 0, 0, 0, 0 }, s2[4] = { 0, 0, 0, 0 };
#pragma unroll
		for (int j = 0; j < 3; j++) {
			const unsigned int *row = lds + (ty + j) * row_dwords + t;
#pragma unroll
			for (int i = 0; i < 3; i++) {
				const int k1 = m.c1[3 * j + i], k2 = m.c2[3 * j + i];
				if (k1 == 0 && k2 == 0) // (wave-uniform)
					continue;
				const int o = lead + i * a.bands;
				const unsigned long long both = ((unsigned long long) row[(o >> 2) + 1] << 32) | row[o >> 2];
				const unsigned int v = (unsigned int) (both >> (8 * (o & 3)));
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const int b = (int) ((v >> (8 * k)) & 255u);
					s1[k] += k1 * b;
					s2[k] += k2 * b;
				}
			}
		}
		unsigned int acc = 0;
#pragma unroll
		for (int k = 0; k < 4; k++)
			acc |= edge_uchar(edge_conv_clip(s1[k]), edge_conv_clip(s2[k])) << (8 * k);
		if (e < out_elems) {
			const unsigned long long p = (unsigned long long) a.out + (unsigned long long) (y0 + ty) * (unsigned long long) a.out_stride +
				(unsigned long long) e;
			if ((p & 3) == 0 && e + 4 <= out_elems)
				gstore32(gptr_out_of(p), acc);
			else {
#pragma unroll
				for (int k = 0; k < 4; k++)
					if (e + k < out_elems)
						gstore8(gptr_out_of(p + k), (unsigned char) (acc >> (8 * k)));
			}
		}
	}
}

// bytes of a staged row: the lead of the rounding, the tile, the halo, the dword behind the last one read
static long long edge_lds_row(int bands)
{
	return (3 + EDGE_TW + 2LL * bands + 4 + 15) / 16 * 16;
}

int edge_u8_fits(int bands)
{
	return edge_lds_row(bands) * (EDGE_TH + 2) <= EDGE_LDS_MAX;
}

// Everything about the regions has been checked (ops_edge.cpp); win_w == win_h == 3.
int edge_u8_run(const char *domain, NbArgs a, const int *mask, const int *mask90)
{
	if (a.win_w != 3 || a.win_h != 3 || !edge_u8_fits(a.bands)) {
		error(domain, "the fused kernel takes 3 x 3 masks and pels of up to %d bands", edge_tile(2));
		return -1;
	}
	EdgeArgs m = {};
	a.lds_row = (int) edge_lds_row(a.bands);
	a.key_xor = 0;
	a.index = 0;
	m.nb = a;
	for (int i = 0; i < 9; i++) {
		// |sum| stays far inside an int: 9 x 255 x |c|
		if (mask[i] < -100000 || mask[i] > 100000) {
			error(domain, "mask element %d out of range", mask[i]);
			return -1;
		}
		m.c1[i] = mask[i];
		m.c2[i] = mask90[i];
	}
	const long long lds = (long long) a.lds_row * (EDGE_TH + 2);
	const long long out_elems = (long long) a.out_width * a.bands;
	const dim3 grid((unsigned int) ((out_elems + EDGE_TW - 1) / EDGE_TW), (unsigned int) ((a.out_height + EDGE_TH - 1) / EDGE_TH), 1);
	{
		Gate gate("edge_u8");
		hipLaunchKernelGGL(edge_u8_kernel, grid, dim3(EDGE_THREADS), (size_t) lds, stream(), m);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

int edge_tile(int what)
{
	if (what == 0)
		return EDGE_TW;
	if (what == 1)
		return EDGE_TH;
	if (what == 2) { // the widest pel the fused kernel stages
		int bands = 1;
		while (edge_u8_fits(bands + 1))
			bands++;
		return bands;
	}
	if (what == 3)
		return EDGE_COMBINE_ROWS;
	return 0;
}

// ---- the general tier's tail

struct EdgeCombineArgs {
	const unsigned char *c1, *c2; // the two convolutions, float or uchar
	unsigned char *out;           // uchar
	long long c1_stride, c2_stride, out_stride; // bytes
	int elems, height; // elements a row
};

template <bool FLOAT>
__global__ void __launch_bounds__(EDGE_THREADS)
edge_combine_kernel(EdgeCombineArgs a)
{
	for (int y = (int) blockIdx.y; y < a.height; y += (int) gridDim.y) {
		const unsigned char *r1 = a.c1 + (long long) y * a.c1_stride;
		const unsigned char *r2 = a.c2 + (long long) y * a.c2_stride;
		unsigned char *q = a.out + (long long) y * a.out_stride;
		for (int x = (int) (blockIdx.x * EDGE_THREADS) + tid(); x < a.elems; x += (int) gridDim.x * EDGE_THREADS) {
			if constexpr (FLOAT) {
				const float p1 = ((const float *) r1)[x], p2 = ((const float *) r2)[x];
				const float sum = __fadd_rn(__fmul_rn(p1, p1), __fmul_rn(p2, p2));
				const float root = sum == 0.0f ? 0.0f : (float) sqrt((double) sum);
				double d = (double) root;
				d = 255.0 < d ? 255.0 : d;
				d = 0.0 > d ? 0.0 : d;
				q[x] = (unsigned char) cvt_i32(d);
			}
			else
				q[x] = (unsigned char) edge_uchar(r1[x], r2[x]);
		}
	}
}

// `c1` and `c2` hold the out rect's rows of the two convolutions (float: is_float, else uchar); `out` is the uchar rect.
int edge_combine_run(const char *domain, const void *c1, long long c1_stride, const void *c2, long long c2_stride, void *out,
	long long out_stride, long long elems, int height, int is_float)
{
	if (elems <= 0 || height <= 0)
		return 0;
	if (elems >= (1LL << 31)) {
		error(domain, "image too large");
		return -1;
	}
	EdgeCombineArgs a = {};
	a.c1 = (const unsigned char *) c1;
	a.c2 = (const unsigned char *) c2;
	a.out = (unsigned char *) out;
	a.c1_stride = c1_stride;
	a.c2_stride = c2_stride;
	a.out_stride = out_stride;
	a.elems = (int) elems;
	a.height = height;
	long long blocks = (elems + EDGE_THREADS - 1) / EDGE_THREADS;
	blocks = blocks > 4096 ? 4096 : blocks;
	const dim3 grid((unsigned int) blocks, (unsigned int) (height > EDGE_COMBINE_ROWS ? EDGE_COMBINE_ROWS : height), 1);
	{
		Gate gate(is_float ? "edge_combine_f32" : "edge_combine_u8");
		if (is_float)
			hipLaunchKernelGGL(edge_combine_kernel<true>, grid, dim3(EDGE_THREADS), 0, stream(), a);
		else
			hipLaunchKernelGGL(edge_combine_kernel<false>, grid, dim3(EDGE_THREADS), 0, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

// ---- vips_compass (convolution/compass.c)

constexpr int COMPASS_MASKS = 8; // rot45 of an odd square matrix has period 8

struct CompassArgs {
	NbArgs nb;
	int n;                       // distinct masks, 1 .. COMPASS_MASKS
	int scale, rounding, offset; // of every convolution (rot45 carries them along)
	int mult[COMPASS_MASKS];     // how many of the `times` convolutions run mask k (sum)
	int c[COMPASS_MASKS][9];
};

// vips_convi_gen's tail for uchar, convi.c:712 (the reference sums in 64 bits; the host keeps the sums inside 32)
template <bool SCALE1>
VH_DEV int compass_conv_clip(int sum, int scale, int rounding, int offset)
{
	const int v = (SCALE1 ? sum : (sum + rounding) / scale) + offset;
	return v < 0 ? 0 : v > 255 ? 255 : v;
}

// The fused kernel for uchar with precision integer and 3 x 3 masks: every mask's integer convolution, clipped as the
// library stores it, from ONE staged tile (the tile and the lane's dword are edge_u8's); vips_abs of a uchar image is
// a copy (abs.c:88-90); then vips_bandrank's max or min (uchar out) or vips_sum (uint out, sum.c:90).  The nine
// shifted dwords of an output row are read once and every mask runs over them; the masks are indexed by constants only.
// COMBINE: 0 max, 1 sum, 2 min (VipsCombine).
template <int COMBINE, bool SCALE1>
__global__ void __launch_bounds__(EDGE_THREADS)
compass_u8_kernel(CompassArgs m)
{
	VH_DYNAMIC_LDS(unsigned int, lds);
	const NbArgs &a = m.nb;

	const int out_e0 = a.out_left * a.bands + (int) blockIdx.x * EDGE_TW;
	const int y0 = (int) blockIdx.y * EDGE_TH;
	const int s = out_e0 - a.bands;
	const int s_al = s & ~3;
	const int lead = s - s_al;
	nb_stage<1, false>(a, lds, s_al, a.out_top + y0 - 1, EDGE_TH + 2, EDGE_THREADS);
	barrier();

	const int t = tid();
	const int e = (int) blockIdx.x * EDGE_TW + 4 * t;
	const int out_elems = a.out_width * a.bands;
	const int row_dwords = a.lds_row >> 2;
	for (int ty = 0; ty < EDGE_TH; ty++) {
		if (y0 + ty >= a.out_height)
			break;
		unsigned int v[9];
#pragma unroll
		for (int j = 0; j < 3; j++) {
			const unsigned int *row = lds + (ty + j) * row_dwords + t;
#pragma unroll
			for (int i = 0; i < 3; i++) {
				const int o = lead + i * a.bands;
				const unsigned long long both = ((unsigned long long) row[(o >> 2) + 1] << 32) | row[o >> 2];
				v[3 * j + i] = (unsigned int) (both >> (8 * (o & 3)));
			}
		}
		unsigned int acc[4];
#pragma unroll
		for (int k = 0; k < 4; k++)
			acc[k] = COMBINE == 2 ? 255u : 0u;
#pragma unroll
		for (int n = 0; n < COMPASS_MASKS; n++) {
			if (n < m.n) { // (wave-uniform)
				int sum[4] = { 0, 0, 0, 0 };
#pragma unroll
				for (int tap = 0; tap < 9; tap++) {
					const int c = m.c[n][tap];
					if (c != 0) {
#pragma unroll
						for (int k = 0; k < 4; k++)
							sum[k] += c * (int) ((v[tap] >> (8 * k)) & 255u);
					}
				}
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const unsigned int p = (unsigned int) compass_conv_clip<SCALE1>(sum[k], m.scale, m.rounding, m.offset);
					if (COMBINE == 0)
						acc[k] = p > acc[k] ? p : acc[k];
					else if (COMBINE == 2)
						acc[k] = p < acc[k] ? p : acc[k];
					else
						acc[k] += (unsigned int) m.mult[n] * p;
				}
			}
		}
		if (e < out_elems) {
			if (COMBINE == 1) { // uint elements
				const unsigned long long p = (unsigned long long) a.out + (unsigned long long) (y0 + ty) * (unsigned long long) a.out_stride +
					4ull * (unsigned long long) e;
				if (e + 4 <= out_elems)
					gstore128(gptr_out_of(p), acc);
				else {
#pragma unroll
					for (int k = 0; k < 4; k++)
						if (e + k < out_elems)
							gstore32(gptr_out_of(p + 4 * k), acc[k]);
				}
			}
			else {
				const unsigned int packed = acc[0] | (acc[1] << 8) | (acc[2] << 16) | (acc[3] << 24);
				const unsigned long long p = (unsigned long long) a.out + (unsigned long long) (y0 + ty) * (unsigned long long) a.out_stride +
					(unsigned long long) e;
				if ((p & 3) == 0 && e + 4 <= out_elems)
					gstore32(gptr_out_of(p), packed);
				else {
#pragma unroll
					for (int k = 0; k < 4; k++)
						if (e + k < out_elems)
							gstore8(gptr_out_of(p + k), (unsigned char) (packed >> (8 * k)));
				}
			}
		}
	}
}

template <int COMBINE>
static void compass_u8_launch(const CompassArgs &m, dim3 grid, size_t lds)
{
	if (m.scale == 1)
		hipLaunchKernelGGL((compass_u8_kernel<COMBINE, true>), grid, dim3(EDGE_THREADS), lds, stream(), m);
	else
		hipLaunchKernelGGL((compass_u8_kernel<COMBINE, false>), grid, dim3(EDGE_THREADS), lds, stream(), m);
}

// Can the fused kernel run these masks?  Its sums are ints: 9 x 255 x |c| + |rounding| must stay inside one.
int compass_u8_takes(int bands, const int *masks, int n, int scale)
{
	if (!edge_u8_fits(bands) || n < 1 || n > COMPASS_MASKS || scale == 0 || scale > (1 << 28) || scale < -(1 << 28))
		return 0;
	for (int i = 0; i < 9 * n; i++)
		if (masks[i] < -100000 || masks[i] > 100000)
			return 0;
	return 1;
}

// Everything about the regions has been checked (ops_edge.cpp); `masks` n x 9 ints, `mult` n counts (their sum at most
// 1000: a sum stays far below 2^32); `out` is uchar for max and min, uint for sum.
int compass_u8_run(const char *domain, NbArgs a, const int *masks, const int *mult, int n, int scale, int offset, int combine)
{
	if (a.win_w != 3 || a.win_h != 3 || !compass_u8_takes(a.bands, masks, n, scale) || combine < 0 || combine > 2) {
		error(domain, "not a case of the fused kernel");
		return -1;
	}
	CompassArgs m = {};
	a.lds_row = (int) edge_lds_row(a.bands);
	a.key_xor = 0;
	a.index = 0;
	m.nb = a;
	m.n = n;
	m.scale = scale;
	m.rounding = scale / 2;
	m.offset = offset;
	for (int k = 0; k < n; k++) {
		m.mult[k] = mult[k];
		for (int i = 0; i < 9; i++)
			m.c[k][i] = masks[9 * k + i];
	}
	const size_t lds = (size_t) a.lds_row * (EDGE_TH + 2);
	const long long out_elems = (long long) a.out_width * a.bands;
	const dim3 grid((unsigned int) ((out_elems + EDGE_TW - 1) / EDGE_TW), (unsigned int) ((a.out_height + EDGE_TH - 1) / EDGE_TH), 1);
	{
		Gate gate("compass_u8");
		if (combine == 0)
			compass_u8_launch<0>(m, grid, lds);
		else if (combine == 1)
			compass_u8_launch<1>(m, grid, lds);
		else
			compass_u8_launch<2>(m, grid, lds);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

// The general tier's tail: vips_abs of every convolution (abs.c:100-120), then vips_bandrank's max / min
// (bandrank.c:75-105, in the convolutions' format) or vips_sum (sum.c:56-69: summed in the OUTPUT type, image after
// image in their order -- a float sum is not reordered, so the `times` terms are walked through the `n` planes).
struct CompassCombineArgs {
	const unsigned char *in; // n planes of height rows, one a distinct mask's convolution
	unsigned char *out;
	long long in_stride, plane, out_stride; // bytes
	int elems, height, n, times;
};

template <typename T>
VH_DEV T compass_abs(T v)
{
	if constexpr (std::is_floating_point<T>::value)
		return fabsf(v);
	else if constexpr (std::is_unsigned<T>::value)
		return v;
	else
		return (T) (v < 0 ? 0u - (unsigned int) (int) v : (unsigned int) (int) v); // (the type's minimum stays itself)
}

template <typename T, typename TS, int COMBINE>
__global__ void __launch_bounds__(EDGE_THREADS)
compass_combine_kernel(CompassCombineArgs a)
{
	for (int y = (int) blockIdx.y; y < a.height; y += (int) gridDim.y) {
		const unsigned char *r = a.in + (long long) y * a.in_stride;
		unsigned char *q = a.out + (long long) y * a.out_stride;
		for (int x = (int) (blockIdx.x * EDGE_THREADS) + tid(); x < a.elems; x += (int) gridDim.x * EDGE_THREADS) {
			if constexpr (COMBINE == 1) {
				TS sum = (TS) compass_abs(((const T *) r)[x]);
				for (int i = 1, k = 1; i < a.times; i++, k++) {
					k = k == a.n ? 0 : k;
					const TS v = (TS) compass_abs(((const T *) (r + (long long) k * a.plane))[x]);
					if constexpr (std::is_floating_point<TS>::value)
						sum = __fadd_rn(sum, v);
					else
						sum += v;
				}
				((TS *) q)[x] = sum;
			}
			else {
				T best = compass_abs(((const T *) r)[x]);
				for (int k = 1; k < a.n; k++) {
					const T v = compass_abs(((const T *) (r + (long long) k * a.plane))[x]);
					if (COMBINE == 0 ? v > best : v < best)
						best = v;
				}
				((T *) q)[x] = best;
			}
		}
	}
}

template <typename T, typename TS>
static void compass_combine_launch(const CompassCombineArgs &a, dim3 grid, int combine)
{
	if (combine == 0)
		hipLaunchKernelGGL((compass_combine_kernel<T, TS, 0>), grid, dim3(EDGE_THREADS), 0, stream(), a);
	else if (combine == 1)
		hipLaunchKernelGGL((compass_combine_kernel<T, TS, 1>), grid, dim3(EDGE_THREADS), 0, stream(), a);
	else
		hipLaunchKernelGGL((compass_combine_kernel<T, TS, 2>), grid, dim3(EDGE_THREADS), 0, stream(), a);
}

// `in`: n planes (`plane` bytes apart) of the out rect's rows in `format`; `out`: that format for max and min, the
// format vips_sum gives for sum.
int compass_combine_run(const char *domain, const void *in, long long in_stride, long long plane, int n, int times, int format,
	int combine, void *out, long long out_stride, long long elems, int height)
{
	if (elems <= 0 || height <= 0)
		return 0;
	if (elems >= (1LL << 31) || n < 1 || times < n || combine < 0 || combine > 2) {
		error(domain, "image too large");
		return -1;
	}
	CompassCombineArgs a = {};
	a.in = (const unsigned char *) in;
	a.out = (unsigned char *) out;
	a.in_stride = in_stride;
	a.plane = plane;
	a.out_stride = out_stride;
	a.elems = (int) elems;
	a.height = height;
	a.n = n;
	a.times = times;
	long long blocks = (elems + EDGE_THREADS - 1) / EDGE_THREADS;
	blocks = blocks > 4096 ? 4096 : blocks;
	const dim3 grid((unsigned int) blocks, (unsigned int) (height > EDGE_COMBINE_ROWS ? EDGE_COMBINE_ROWS : height), 1);
	{
		Gate gate("compass_combine");
		switch (format) {
		case VIPS_HIP_FORMAT_UCHAR: compass_combine_launch<unsigned char, unsigned int>(a, grid, combine); break;
		case VIPS_HIP_FORMAT_CHAR: compass_combine_launch<signed char, int>(a, grid, combine); break;
		case VIPS_HIP_FORMAT_USHORT: compass_combine_launch<unsigned short, unsigned int>(a, grid, combine); break;
		case VIPS_HIP_FORMAT_SHORT: compass_combine_launch<short, int>(a, grid, combine); break;
		case VIPS_HIP_FORMAT_UINT: compass_combine_launch<unsigned int, unsigned int>(a, grid, combine); break;
		case VIPS_HIP_FORMAT_INT: compass_combine_launch<int, int>(a, grid, combine); break;
		case VIPS_HIP_FORMAT_FLOAT: compass_combine_launch<float, float>(a, grid, combine); break;
		default:
			error(domain, "format %d is outside the HIP path", format);
			return -1;
		}
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

// ---- vips_canny (convolution/canny.c): the 2 x 2 gradient pair, the polar image and the thinning in one kernel

constexpr int CANNY_TW = 64; // pels
constexpr int CANNY_TH = 16; // rows
constexpr int CANNY_LDS_MAX = 160 * 1024;


// dword `index` (per lane) of the atan2 table, from the kernel argument segment
VH_DEV unsigned int canny_table_word(int index)
{
	typedef const unsigned int __attribute__((address_space(4))) *Words;
	const Words w = (Words) ((const char __attribute__((address_space(4))) *) __builtin_amdgcn_kernarg_segment_ptr() +
		offsetof(CannyArgs, atan2_table));
	return w[index];
}

// element `band` of the blurred pel (x, y), as convf reads it: the value of its format as a double.  (x, y) is inside
// the image; it is clamped to the window once more so that nothing outside the window is ever touched.
VH_DEV double canny_at(const CannyArgs &a, int x, int y, int band)
{
	x = nb_clamp(x, a.in_left, a.in_left + a.in_width - 1);
	y = nb_clamp(y, a.in_top, a.in_top + a.in_height - 1);
	const unsigned char *row = a.in + (long long) (y - a.in_top) * a.in_stride;
	const long long e = (long long) (x - a.in_left) * a.bands + band;
	switch (a.format) {
	case VIPS_HIP_FORMAT_UCHAR: return (double) row[e];
	case VIPS_HIP_FORMAT_CHAR: return (double) ((const signed char *) row)[e];
	case VIPS_HIP_FORMAT_USHORT: return (double) ((const unsigned short *) row)[e];
	case VIPS_HIP_FORMAT_SHORT: return (double) ((const short *) row)[e];
	case VIPS_HIP_FORMAT_UINT: return (double) ((const unsigned int *) row)[e];
	case VIPS_HIP_FORMAT_INT: return (double) ((const int *) row)[e];
	default: return (double) ((const float *) row)[e];
	}
}

// POLAR(float)'s theta (canny.c:144-147) from atan2's result
VH_DEV float canny_theta(double angle)
{
	const double theta = (angle / (2.0 * 3.14159265358979323846)) * 360.0; // VIPS_DEG
	return (float) (256.0 * fmod(theta + 360.0, 360.0) / 360.0);
}

// `ulps` steps of a double along its bit pattern (away from zero for ulps > 0)
VH_DEV double canny_step(double v, int ulps)
{
	long long bits = __builtin_bit_cast(long long, v);
	if ((bits & 0x7fffffffffffffffLL) < 8) // (next to zero: atan2 of these arguments is exact there)
		return v;
	bits += ulps;
	return __builtin_bit_cast(double, bits);
}

// UCHAR: the blurred image is uchar -- integer gradients with offset 128 and their clip, the atan2 table, integer
// thinning.  Else: float gradients (convf: a double sum in the mask's raster order, stored as float), POLAR(float) in
// double rounded to float, THIN(float) in float with every operation rounded.
// A block makes CANNY_TW pels x CANNY_TH rows.  The (G, theta) image of its pels and a one-pel ring lies in LDS; the
// ring is the polar of the COPY-extended edge PELS (vips_embed of the polar image, canny.c:414), not the polar of
// extended gradients: a ring pel outside the image is the polar pel of the nearest pel inside, gradient and all.
template <bool UCHAR>
__global__ void __launch_bounds__(EDGE_THREADS)
canny_polar_thin_kernel(CannyArgs a)
{
	typedef typename std::conditional<UCHAR, unsigned char, float>::type T;
	VH_DYNAMIC_LDS(unsigned int, lds);
	unsigned char *table = (unsigned char *) lds;
	T *polar = (T *) (lds + CANNY_TABLE / 4); // [CANNY_TH + 2][CANNY_TW + 2][bands][G, theta]

	const int t = tid();
	if (UCHAR && t < CANNY_TABLE / 4)
		lds[t] = canny_table_word(t);
	if (UCHAR)
		barrier();

	const int x0 = a.out_left + (int) blockIdx.x * CANNY_TW, y0 = a.out_top + (int) blockIdx.y * CANNY_TH;
	constexpr int ring_w = CANNY_TW + 2;
	const int n_ring = ring_w * (CANNY_TH + 2) * a.bands;
	unsigned int marginal = 0;
	for (int idx = t; idx < n_ring; idx += EDGE_THREADS) {
		const int pel = idx / a.bands, band = idx - pel * a.bands;
		const int ty = pel / ring_w, tx = pel - ty * ring_w;
		// the pel of the polar image this ring position copies
		const int cx = nb_clamp(x0 + tx - 1, 0, a.im_width - 1), cy = nb_clamp(y0 + ty - 1, 0, a.im_height - 1);
		// the 2 x 2 masks have their origin at (1, 1): the pel, its left and upper neighbours, edges copied
		const int xl = cx > 0 ? cx - 1 : 0, yu = cy > 0 ? cy - 1 : 0;
		const double p00 = canny_at(a, xl, yu, band), p10 = canny_at(a, cx, yu, band);
		const double p01 = canny_at(a, xl, cy, band), p11 = canny_at(a, cx, cy, band);
		if constexpr (UCHAR) {
			// vips_convi_gen, scale 1, offset 128, CLIP_UCHAR; masks -1 1 / -1 1 and its rot90 -1 -1 / 1 1
			const int i00 = cvt_i32(p00), i10 = cvt_i32(p10), i01 = cvt_i32(p01), i11 = cvt_i32(p11); // (uchar values: exact)
			int Gx = -i00 + i10 - i01 + i11 + 128, Gy = -i00 - i10 + i01 + i11 + 128;
			Gx = Gx < 0 ? 0 : Gx > 255 ? 255 : Gx;
			Gy = Gy < 0 ? 0 : Gy > 255 ? 255 : Gy;
			// POLAR_UCHAR, canny.c:111-129
			const int gx = Gx - 128, gy = Gy - 128;
			const int i = ((gx >> 4) & 0xf) | (gy & 0xf0);
			polar[2 * idx] = (unsigned char) ((gx * gx + gy * gy + 256) >> 9);
			polar[2 * idx + 1] = table[i];
		}
		else {
			// vips_convf_gen, convf.c:163-180: sum = offset, then the non-zero elements in raster order
			double sx = 0.0, sy = 0.0;
			sx += -1.0 * p00;
			sx += 1.0 * p10;
			sx += -1.0 * p01;
			sx += 1.0 * p11;
			sy += -1.0 * p00;
			sy += -1.0 * p10;
			sy += 1.0 * p01;
			sy += 1.0 * p11;
			const double gx = (double) (float) sx, gy = (double) (float) sy;
			// POLAR(float), canny.c:134-155
			const double angle = atan2(gx, gy);
			const float theta = canny_theta(angle);
			polar[2 * idx] = (float) ((gx * gx + gy * gy + 256.0) / 512.0);
			polar[2 * idx + 1] = theta;
			// would theta round to another float if atan2's result moved by 4 ulp either way?
			if (canny_theta(canny_step(angle, 4)) != theta || canny_theta(canny_step(angle, -4)) != theta)
				marginal++;
		}
	}
	if (!UCHAR && marginal)
		atomicAdd(a.marginal, marginal);
	barrier();

	// THIN, canny.c:252-284: the eight neighbours, from the top one anticlockwise
	//   1 | 0 | 7
	//   2 | X | 6
	//   3 | 4 | 5
	const int psk = 2 * a.bands, lsk = ring_w * psk;
	const int offset[8] = { psk, 0, lsk, 2 * lsk, 2 * lsk + psk, 2 * lsk + 2 * psk, lsk + 2 * psk, 2 * psk };
	const int n_out = CANNY_TW * CANNY_TH * a.bands;
	for (int idx = t; idx < n_out; idx += EDGE_THREADS) {
		const int pel = idx / a.bands, band = idx - pel * a.bands;
		const int ty = pel / CANNY_TW, tx = pel - ty * CANNY_TW;
		const int x = x0 + tx - a.out_left, y = y0 + ty - a.out_top; // of the out rect
		if (x >= a.out_width || y >= a.out_height)
			continue;
		const T *tp = polar + ty * lsk + tx * psk + 2 * band; // the top-left pel of the 3 x 3
		T G = tp[lsk + psk];
		const T theta = tp[lsk + psk + 1];
		int low_theta;
		if constexpr (UCHAR)
			low_theta = (theta / 32) & 0x7;
		else
			low_theta = cvt_i32(__fdiv_rn(theta, 32.0f)) & 0x7;
		const int high_theta = (low_theta + 1) & 0x7;
		// (offset[] with a run-time index would go to scratch: pick with selects)
		int o_lowa = 0, o_lowb = 0, o_higha = 0, o_highb = 0;
#pragma unroll
		for (int k = 0; k < 8; k++) {
			o_lowa = low_theta == k ? offset[k] : o_lowa;
			o_lowb = high_theta == k ? offset[k] : o_lowb;
			o_higha = ((low_theta + 4) & 0x7) == k ? offset[k] : o_higha;
			o_highb = ((high_theta + 4) & 0x7) == k ? offset[k] : o_highb;
		}
		const T lowa = tp[o_lowa], lowb = tp[o_lowb], higha = tp[o_higha], highb = tp[o_highb];
		unsigned char *q = a.out + (long long) y * a.out_stride;
		if constexpr (UCHAR) {
			const unsigned char residual = (unsigned char) (theta - low_theta * 32);
			const unsigned char low = (unsigned char) ((lowa * (32 - residual) + lowb * residual) / 32);
			const unsigned char high = (unsigned char) ((higha * (32 - residual) + highb * residual) / 32);
			if (G <= low || G < high)
				G = 0;
			q[x * a.bands + band] = G;
		}
		else {
			const float residual = __fsub_rn(theta, (float) (low_theta * 32));
			const float rest = __fsub_rn(32.0f, residual);
			const float low = __fdiv_rn(__fadd_rn(__fmul_rn(lowa, rest), __fmul_rn(lowb, residual)), 32.0f);
			const float high = __fdiv_rn(__fadd_rn(__fmul_rn(higha, rest), __fmul_rn(highb, residual)), 32.0f);
			if (G <= low || G < high)
				G = 0;
			((float *) q)[x * a.bands + band] = G;
		}
	}
}

static long long canny_lds(int bands, int uchar)
{
	return CANNY_TABLE + (long long) (CANNY_TW + 2) * (CANNY_TH + 2) * bands * 2 * (uchar ? 1 : 4);
}

int canny_tile(int what)
{
	return what == 0 ? CANNY_TW : what == 1 ? CANNY_TH : what == 2 ? (int) ((CANNY_LDS_MAX - CANNY_TABLE) / ((CANNY_TW + 2) * (CANNY_TH + 2) * 8)) : 0;
}

// `a` is filled and checked (ops_edge.cpp) but for the table; uchar: a.format is uchar and `table` holds the 256 bytes
// of vips_atan2_init.
int canny_run(const char *domain, CannyArgs a, const unsigned char *table)
{
	const int uchar = a.format == VIPS_HIP_FORMAT_UCHAR;
	const long long lds = canny_lds(a.bands, uchar);
	if (lds > CANNY_LDS_MAX) {
		error(domain, "pels of %d bands: the kernel takes up to %d", a.bands, canny_tile(2));
		return -1;
	}
	if (a.out_width <= 0 || a.out_height <= 0)
		return 0;
	if (a.out_height > 65535 * CANNY_TH || (long long) a.im_width * a.bands >= (1LL << 28)) {
		error(domain, "image too large");
		return -1;
	}
	if (uchar)
		memcpy(a.atan2_table, table, CANNY_TABLE);
	const dim3 grid((unsigned int) ((a.out_width + CANNY_TW - 1) / CANNY_TW), (unsigned int) ((a.out_height + CANNY_TH - 1) / CANNY_TH), 1);
	const auto kernel = uchar ? canny_polar_thin_kernel<true> : canny_polar_thin_kernel<false>;
	if (lds > 64 * 1024)
		VH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CANNY_LDS_MAX));
	{
		Gate gate(uchar ? "canny_polar_thin_u8" : "canny_polar_thin_f32");
		hipLaunchKernelGGL(kernel, grid, dim3(EDGE_THREADS), (size_t) lds, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

} // namespace vh
