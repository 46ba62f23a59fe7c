// vips_embed, vips_gravity, vips_insert and vips_join (conversion/embed.c, insert.c, join.c), vips_flatten
// (conversion/flatten.c) and vips_addalpha (conversion/addalpha.c) on the device (gfx950).
//
// The canvas family is data movement: canvas pel (X, Y) is
//
//   the sub-image's pel          where the sub-image lies (vips_insert: sub wins)
//   the main image's pel         where the main image lies
//   the ink                      elsewhere, for extend black / white / background and for vips_insert's background
//   the main image's pel at the clamped (copy), clock-arithmetic (repeat, embed.c:378-396) or reflected (mirror,
//   embed.c:398-431: period twice the size, the edge pel repeated) coordinate otherwise
//
// ONE launch an operation writes every byte of the rect once: there is no memset-then-copy pair.
//
//   canvas_stream<P>  lanes on consecutive 16-byte groups of an output row (48 for 3-, 6- and 12-byte pels: whole pels
//                     AND whole 16-byte groups), rows that start on dwords on every side.  A group that lies wholly in
//                     one image is its source group: that starts at (x * P) bytes into the source row, anywhere, so
//                     the lane loads the aligned dwords round it (global_load_dwordx4, one dword more when the group
//                     is not dword aligned) and shifts them into place; a group wholly in the ink is the ink's bytes
//                     from the kernel's arguments, no load.  A group that straddles an edge, lies in a copy / repeat /
//                     mirror border or is the row's ragged end goes pel by pel INSIDE the same kernel (the general
//                     kernel's source function, byte loads), so the launch stays one.
//   canvas_general    one pel a lane, any pel size up to 32 bytes, every mode: defines correctness, takes rows that
//                     do not start on dwords, 24- and 32-byte pels, and everything under VIPS_HIP_NO_CANVAS_STREAM.
//
// flatten: flatten_u8 (the float tables of flatten.c:170-225 / :290-355 in LDS, made per block with the reference's
// own double division; four RGBA pels a lane as dwords where rows start on dwords) and flatten_any<T> (the double
// macros, :88-165).  The file is compiled with -ffp-contract=off: multiply and add stay separate, as in the
// reference's baseline x86-64 code.
#include "pointwise.h"

namespace vh {

constexpr int CANVAS_THREADS = POINTWISE_THREADS;

constexpr int canvas_group_of(int pel) { return 16 % pel == 0 ? 16 : (48 % pel == 0 ? 48 : 0); }

// byte i of the ink (i a constant once the loops are unrolled)
VH_DEV unsigned int canvas_ink_byte(const CanvasArgs &a, int i) { return (a.ink[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// where canvas pel (X, Y) comes from: its address, 0 for the ink
VH_DEV unsigned long long canvas_source(const CanvasArgs &a, int X, int Y)
{
	if (a.sub) {
		const int u = X - a.sx, v = Y - a.sy;
		if ((unsigned int) u < (unsigned int) a.sw && (unsigned int) v < (unsigned int) a.sh)
			return (unsigned long long) a.sub + (unsigned long long) v * a.sub_stride + (unsigned long long) u * a.pel;
	}
	int ix = X - a.mx, iy = Y - a.my;
	if ((unsigned int) ix >= (unsigned int) a.mw || (unsigned int) iy >= (unsigned int) a.mh) {
		switch (a.mode) {
		case CANVAS_COPY:
			ix = ix < 0 ? 0 : (ix > a.mw - 1 ? a.mw - 1 : ix);
			iy = iy < 0 ? 0 : (iy > a.mh - 1 ? a.mh - 1 : iy);
			break;
		case CANVAS_REPEAT:
			ix %= a.mw;
			iy %= a.mh;
			ix += ix < 0 ? a.mw : 0;
			iy += iy < 0 ? a.mh : 0;
			break;
		case CANVAS_MIRROR: {
			const int w2 = 2 * a.mw, h2 = 2 * a.mh;
			ix %= w2;
			iy %= h2;
			ix += ix < 0 ? w2 : 0;
			iy += iy < 0 ? h2 : 0;
			ix = ix < a.mw ? ix : w2 - 1 - ix;
			iy = iy < a.mh ? iy : h2 - 1 - iy;
			break;
		}
		default:
			return 0;
		}
	}
	return (unsigned long long) a.main + (unsigned long long) (iy - a.win_top) * a.main_stride +
		(unsigned long long) (ix - a.win_left) * a.pel;
}

// ---------------------------------------------------------------- one pel a lane

template <typename UT>
__global__ void __launch_bounds__(CANVAS_THREADS)
canvas_general_kernel(CanvasArgs a)
{
	const int ox = (int) blockIdx.x * CANVAS_THREADS + (int) threadIdx.x;
	if (ox >= a.out_width)
		return;
	const int units = a.pel / (int) sizeof(UT);
	for (int oy = (int) blockIdx.y; oy < a.out_height; oy += (int) gridDim.y) {
		const unsigned long long from = canvas_source(a, a.out_left + ox, a.out_top + oy);
		UT *dst = (UT *) (a.out + (long long) oy * a.out_stride + (long long) ox * a.pel);
		if (from) {
			const UT *src = (const UT *) from;
			for (int i = 0; i < units; i++)
				dst[i] = src[i];
		}
		else {
			for (int i = 0; i < units; i++) {
				UT v;
				if constexpr (sizeof(UT) == 8)
					v = (UT) a.ink[2 * i] | ((UT) a.ink[2 * i + 1] << 32);
				else
					v = (UT) (a.ink[i * (int) sizeof(UT) / 4] >> (8 * ((i * (int) sizeof(UT)) & 3)));
				dst[i] = v;
			}
		}
	}
}

// ---------------------------------------------------------------- 16 / 48 bytes a lane

template <int P>
__global__ void __launch_bounds__(CANVAS_THREADS)
canvas_stream_kernel(CanvasArgs a)
{
	constexpr int NB = canvas_group_of(P);
	constexpr int NP = NB / P, ND = NB / 4;
	// the rect's groups, rows after rows, dealt to the lanes as ONE sequence: a row of groups is rarely a whole number
	// of blocks, and lanes past a row's end would idle for the whole launch
	const unsigned int total = (unsigned int) a.groups * (unsigned int) a.out_height;
	for (unsigned int at = (unsigned int) blockIdx.x * CANVAS_THREADS + (unsigned int) threadIdx.x; at < total; at += (unsigned int) gridDim.x * CANVAS_THREADS) {
		const int y = (int) (at / (unsigned int) a.groups);
		const int g = (int) (at - (unsigned int) y * (unsigned int) a.groups);
		const int p0 = g * NP; // the group's first pel, in the rect
		const int X0 = a.out_left + p0;
		const int npel = min(NP, a.out_width - p0); // < NP: the row's ragged end
		const bool whole = npel == NP;
		const bool cols_in_main = whole && X0 >= a.mx && X0 + NP <= a.mx + a.mw;
		const bool cols_off_main = X0 + npel <= a.mx || X0 >= a.mx + a.mw;
		const bool cols_in_sub = a.sub && whole && X0 >= a.sx && X0 + NP <= a.sx + a.sw;
		const bool cols_off_sub = !a.sub || X0 + npel <= a.sx || X0 >= a.sx + a.sw;
		const int Y = a.out_top + y;
		const bool row_in_sub = a.sub && (unsigned int) (Y - a.sy) < (unsigned int) a.sh;
		const bool row_in_main = (unsigned int) (Y - a.my) < (unsigned int) a.mh;
		const gptr_out ob = gptr_out_of((unsigned long long) a.out + (unsigned long long) y * a.out_stride) + (unsigned int) g * NB;
		unsigned int w[ND];
		unsigned long long src = 0;
		bool ink = false;
		if (row_in_sub && cols_in_sub)
			src = (unsigned long long) a.sub + (unsigned long long) (Y - a.sy) * a.sub_stride + (unsigned long long) (X0 - a.sx) * P;
		else if (whole && (!row_in_sub || cols_off_sub)) {
			if (row_in_main && cols_in_main)
				src = (unsigned long long) a.main + (unsigned long long) (Y - a.my - a.win_top) * a.main_stride +
					(unsigned long long) (X0 - a.mx - a.win_left) * P;
			else if (a.mode == CANVAS_INK && (!row_in_main || cols_off_main))
				ink = true;
		}
		if (src) {
			// the aligned dwords round the source group, shifted: rows start on dwords, so the last of them -- up to
			// 3 bytes past the group -- ends inside the source row's stride (vips_hip_embed_gen states that a
			// region's memory covers height * stride)
			const unsigned int sh = (unsigned int) src & 3u;
			const gptr_in ib = gptr_in_of(src - sh);
			unsigned int d[ND + 1];
#pragma unroll
			for (int q = 0; q < ND / 4; q++) {
				unsigned int t[4];
				gload128(ib, 16 * q, t);
#pragma unroll
				for (int i = 0; i < 4; i++)
					d[4 * q + i] = t[i];
			}
			d[ND] = 0;
			if (sh)
				d[ND] = gload32(ib, NB);
#pragma unroll
			for (int i = 0; i < ND; i++)
				w[i] = (unsigned int) ((((unsigned long long) d[i + 1] << 32) | d[i]) >> (8 * sh));
		}
		else if (ink) {
#pragma unroll
			for (int i = 0; i < ND; i++)
				w[i] = canvas_ink_byte(a, (4 * i) % P) | (canvas_ink_byte(a, (4 * i + 1) % P) << 8) |
					(canvas_ink_byte(a, (4 * i + 2) % P) << 16) | (canvas_ink_byte(a, (4 * i + 3) % P) << 24);
		}
		else {
			// pel by pel: an edge inside the group, a copy / repeat / mirror border, the ragged end
#pragma unroll
			for (int i = 0; i < ND; i++)
				w[i] = 0;
#pragma unroll
			for (int j = 0; j < NP; j++) {
				if (j < npel) {
					const unsigned long long from = canvas_source(a, X0 + j, Y);
#pragma unroll
					for (int b = 0; b < P; b++) {
						const int k = j * P + b;
						const unsigned int v = from ? (unsigned int) *(const unsigned char *) (from + b) : canvas_ink_byte(a, b);
						w[k >> 2] |= v << (8 * (k & 3));
					}
				}
			}
		}
		if (whole) {
#pragma unroll
			for (int q = 0; q < ND / 4; q++) {
				const unsigned int t[4] = { w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3] };
				gstore128(ob + 16 * q, t);
			}
		}
		else {
#pragma unroll
			for (int k = 0; k < NB; k++)
				if (k < npel * P)
					gstore8(ob + k, (unsigned char) (w[k >> 2] >> (8 * (k & 3))));
		}
	}
}

// ---------------------------------------------------------------- dispatch

// the largest of 8, 4, 2, 1 that divides every row start (and the pel size)
static int canvas_unit(const CanvasArgs &a, int most, bool with_pel)
{
	uintptr_t all = (uintptr_t) a.main | (uintptr_t) a.out | (uintptr_t) a.main_stride | (uintptr_t) a.out_stride;
	if (with_pel)
		all |= (uintptr_t) a.pel;
	if (a.sub)
		all |= (uintptr_t) a.sub | (uintptr_t) a.sub_stride;
	int u = most;
	while (u > 1 && all % (uintptr_t) u)
		u >>= 1;
	return u;
}

static void canvas_launch_general(const CanvasArgs &a)
{
	const int bx = (a.out_width + CANVAS_THREADS - 1) / CANVAS_THREADS;
	dim3 grid(bx, pointwise_rows_grid(bx, a.out_height), 1), block(CANVAS_THREADS, 1, 1);
	Gate gate("canvas_general");
	switch (canvas_unit(a, 8, true)) {
	case 8: hipLaunchKernelGGL((canvas_general_kernel<unsigned long long>), grid, block, 0, stream(), a); break;
	case 4: hipLaunchKernelGGL((canvas_general_kernel<unsigned int>), grid, block, 0, stream(), a); break;
	case 2: hipLaunchKernelGGL((canvas_general_kernel<unsigned short>), grid, block, 0, stream(), a); break;
	default: hipLaunchKernelGGL((canvas_general_kernel<unsigned char>), grid, block, 0, stream(), a); break;
	}
}

template <int P>
static void canvas_launch_stream(CanvasArgs a)
{
	constexpr int NP = canvas_group_of(P) / P;
	a.groups = (a.out_width + NP - 1) / NP;
	// enough blocks to fill the part (as many as rot.hip's streams launch), the rest of the groups in turns
	dim3 grid = pointwise_stream_grid((long long) a.groups * a.out_height), block(CANVAS_THREADS, 1, 1);
	Gate gate("canvas_stream");
	hipLaunchKernelGGL((canvas_stream_kernel<P>), grid, block, 0, stream(), a);
}

static bool canvas_stream_ok(const CanvasArgs &a)
{
	if (getenv("VIPS_HIP_NO_CANVAS_STREAM"))
		return false;
	// rows that start on dwords on every side: the aligned dwords round a source group then lie in its row
	if (a.pel > 16 || canvas_group_of(a.pel) == 0 || canvas_unit(a, 4, false) != 4)
		return false;
	// (the kernel numbers the rect's groups in 32 bits)
	const long long groups = (a.out_width + (long long) canvas_group_of(a.pel) / a.pel - 1) / (canvas_group_of(a.pel) / a.pel);
	return groups * a.out_height < (1LL << 31);
}

int canvas_tile(int what, int pel)
{
	switch (what) {
	case 0: return CANVAS_THREADS;
	case 1: return pel >= 1 && pel <= 16 ? canvas_group_of(pel) : 0;
	case 2: return POINTWISE_GRID_BLOCKS;
	default: return 0;
	}
}

int canvas_run(const char *domain, CanvasArgs a)
{
	if (a.pel < 1 || a.pel > CANVAS_MAX_PEL) {
		error(domain, "pels of more than %d bytes are outside the HIP path", CANVAS_MAX_PEL);
		return -1;
	}
	// the kernels work out coordinates in int: positions within +- 10^9 and sizes up to 10^9 (the range of vips_embed's
	// arguments) keep every difference, every position + size and twice a size (mirror) inside it
	constexpr int LIMIT = 1000000000;
	const int sizes[] = { a.mw, a.mh, a.sw, a.sh, a.out_width, a.out_height };
	const int positions[] = { a.mx, a.my, a.sx, a.sy, a.out_left, a.out_top, a.win_left, a.win_top };
	for (int v : sizes)
		if (v < 0 || v > LIMIT) {
			error(domain, "image size out of range");
			return -1;
		}
	for (int v : positions)
		if (v < -LIMIT || v > LIMIT) {
			error(domain, "position out of range");
			return -1;
		}
	if ((long long) a.out_width * a.pel >= (1LL << 31) || (long long) a.mw * a.pel >= (1LL << 31) ||
		(long long) a.sw * a.pel >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	if (canvas_stream_ok(a)) {
		switch (a.pel) {
#define GO(P) \
	case P: \
		canvas_launch_stream<P>(a); \
		VH_CHECK(hipGetLastError()); \
		return 0;
			GO(1) GO(2) GO(3) GO(4) GO(6) GO(8) GO(12) GO(16)
#undef GO
		default: break;
		}
	}
	canvas_launch_general(a);
	VH_CHECK(hipGetLastError());
	return 0;
}

// ---------------------------------------------------------------- flatten

constexpr int FLATTEN_THREADS = 256;

// flatten.c:183-185 / :306-311: (float) (i / max_alpha) and (float) ((max_alpha - i) / max_alpha), the division in
// double and correctly rounded, as the reference's
VH_DEV void flatten_tables(float *fa, float *fn, double max_alpha)
{
	const int i = (int) threadIdx.x;
	fa[i] = (float) ((double) i / max_alpha);
	fn[i] = (float) ((max_alpha - (double) i) / max_alpha);
	__syncthreads();
}

// one band: q = p * fa [+ bg * fn], float arithmetic, then the conversion to uchar (in range: the tables are at most 1)
VH_DEV unsigned int flatten_u8_band(unsigned int p, float fa, unsigned int bg, float fn, bool black)
{
	const float v = black ? (float) (int) p * fa : (float) (int) p * fa + (float) (int) bg * fn;
	return (unsigned int) cvt_i32(v) & 0xffu;
}

// QUAD: four RGBA pels a lane, 16 bytes in and 12 out as dwords (rows start on dwords); otherwise one pel a lane
template <bool QUAD>
__global__ void __launch_bounds__(FLATTEN_THREADS)
flatten_u8_kernel(FlattenArgs a)
{
	__shared__ float fa[256], fn[256];
	flatten_tables(fa, fn, a.max_alpha);
	const int lane = (int) blockIdx.x * FLATTEN_THREADS + (int) threadIdx.x;
	const unsigned char *bg = (const unsigned char *) a.ink;
	if constexpr (QUAD) {
		const int x = 4 * lane;
		if (x >= a.width)
			return;
		const unsigned int bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];
		for (int y = (int) blockIdx.y; y < a.height; y += (int) gridDim.y) {
			const gptr_in ib = gptr_in_of((unsigned long long) a.in + (unsigned long long) y * a.in_stride);
			const gptr_out ob = gptr_out_of((unsigned long long) a.out + (unsigned long long) y * a.out_stride) + (unsigned int) (3 * x);
			if (x + 4 <= a.width) {
				unsigned int p[4], q[4];
				gload128(ib, 4u * (unsigned int) x, p);
#pragma unroll
				for (int i = 0; i < 4; i++) {
					const float f = fa[p[i] >> 24], n = fn[p[i] >> 24];
					q[i] = flatten_u8_band(p[i] & 0xffu, f, bg0, n, a.black != 0) |
						(flatten_u8_band((p[i] >> 8) & 0xffu, f, bg1, n, a.black != 0) << 8) |
						(flatten_u8_band((p[i] >> 16) & 0xffu, f, bg2, n, a.black != 0) << 16);
				}
				const unsigned int w[3] = { q[0] | (q[1] << 24), (q[1] >> 8) | (q[2] << 16), (q[2] >> 16) | (q[3] << 8) };
				gstore_dwords<3>(ob, w);
			}
			else {
				for (int i = 0; x + i < a.width; i++) {
					const unsigned int p = gload32(ib, 4u * (unsigned int) (x + i));
					const float f = fa[p >> 24], n = fn[p >> 24];
					gstore8(ob + 3 * i, (unsigned char) flatten_u8_band(p & 0xffu, f, bg0, n, a.black != 0));
					gstore8(ob + 3 * i + 1, (unsigned char) flatten_u8_band((p >> 8) & 0xffu, f, bg1, n, a.black != 0));
					gstore8(ob + 3 * i + 2, (unsigned char) flatten_u8_band((p >> 16) & 0xffu, f, bg2, n, a.black != 0));
				}
			}
		}
	}
	else {
		const int x = lane;
		if (x >= a.width)
			return;
		const int ob = a.bands - 1;
		for (int y = (int) blockIdx.y; y < a.height; y += (int) gridDim.y) {
			const unsigned char *p = a.in + (long long) y * a.in_stride + (long long) x * a.bands;
			unsigned char *q = a.out + (long long) y * a.out_stride + (long long) x * ob;
			const float f = fa[p[ob]], n = fn[p[ob]];
			for (int b = 0; b < ob; b++)
				q[b] = (unsigned char) flatten_u8_band(p[b], f, a.black ? 0u : (unsigned int) bg[b], n, a.black != 0);
		}
	}
}

// the double macros: VIPS_FLATTEN_BLACK_INT / _BLACK_FLOAT / _INT / _FLOAT (flatten.c:88-165).  The INT forms (char
// images only: uchar takes the tables) multiply and add small integers, which double arithmetic does exactly too, so
// one expression serves; TYPE nalpha = max_alpha - alpha is a conversion of a double to TYPE
template <typename T>
__global__ void __launch_bounds__(FLATTEN_THREADS)
flatten_any_kernel(FlattenArgs a)
{
	const int x = (int) blockIdx.x * FLATTEN_THREADS + (int) threadIdx.x;
	if (x >= a.width)
		return;
	const int ob = a.bands - 1;
	const T *bg = (const T *) a.ink;
	for (int y = (int) blockIdx.y; y < a.height; y += (int) gridDim.y) {
		const T *p = (const T *) (a.in + (long long) y * a.in_stride) + (long long) x * a.bands;
		T *q = (T *) (a.out + (long long) y * a.out_stride) + (long long) x * ob;
		const T alpha = p[ob];
		if (a.black) {
			for (int b = 0; b < ob; b++)
				q[b] = cvt_to<T>(((double) p[b] * (double) alpha) / a.max_alpha);
		}
		else {
			const T nalpha = cvt_to<T>(a.max_alpha - (double) alpha);
			for (int b = 0; b < ob; b++)
				q[b] = cvt_to<T>(((double) p[b] * (double) alpha + (double) bg[b] * (double) nalpha) / a.max_alpha);
		}
	}
}

int flatten_run(const char *domain, FlattenArgs a, int format)
{
	if ((long long) a.width * a.bands * format_sizeof(format) >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	dim3 block(FLATTEN_THREADS, 1, 1);
	if (format == VIPS_HIP_FORMAT_UCHAR) {
		const uintptr_t all = (uintptr_t) a.in | (uintptr_t) a.out | (uintptr_t) a.in_stride | (uintptr_t) a.out_stride;
		const bool quad = a.bands == 4 && all % 4 == 0;
		const int lanes = quad ? (a.width + 3) / 4 : a.width;
		const int bx = (lanes + FLATTEN_THREADS - 1) / FLATTEN_THREADS;
		dim3 grid(bx, pointwise_rows_grid(bx, a.height), 1);
		Gate gate("flatten_u8");
		if (quad)
			hipLaunchKernelGGL((flatten_u8_kernel<true>), grid, block, 0, stream(), a);
		else
			hipLaunchKernelGGL((flatten_u8_kernel<false>), grid, block, 0, stream(), a);
		VH_CHECK(hipGetLastError());
		return 0;
	}
	const int bx = (a.width + FLATTEN_THREADS - 1) / FLATTEN_THREADS;
	dim3 grid(bx, pointwise_rows_grid(bx, a.height), 1);
	Gate gate("flatten_any");
	switch (format) {
#define GO(F, T) \
	case F: hipLaunchKernelGGL((flatten_any_kernel<T>), grid, block, 0, stream(), a); break;
		GO(VIPS_HIP_FORMAT_CHAR, signed char)
		GO(VIPS_HIP_FORMAT_USHORT, unsigned short)
		GO(VIPS_HIP_FORMAT_SHORT, short)
		GO(VIPS_HIP_FORMAT_UINT, unsigned int)
		GO(VIPS_HIP_FORMAT_INT, int)
		GO(VIPS_HIP_FORMAT_FLOAT, float)
		GO(VIPS_HIP_FORMAT_DOUBLE, double)
#undef GO
	default:
		error(domain, "image must be non-complex");
		return -1;
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

// ---------------------------------------------------------------- addalpha

template <typename UT>
__global__ void __launch_bounds__(FLATTEN_THREADS)
addalpha_kernel(const unsigned char *in, long long in_stride, unsigned char *out, long long out_stride, int width, int height,
	int bands, unsigned long long alpha)
{
	const int x = (int) blockIdx.x * FLATTEN_THREADS + (int) threadIdx.x;
	if (x >= width)
		return;
	for (int y = (int) blockIdx.y; y < height; y += (int) gridDim.y) {
		const UT *p = (const UT *) (in + (long long) y * in_stride) + (long long) x * bands;
		UT *q = (UT *) (out + (long long) y * out_stride) + (long long) x * (bands + 1);
		for (int b = 0; b < bands; b++)
			q[b] = p[b];
		q[bands] = (UT) alpha;
	}
}

int addalpha_run(const char *domain, const unsigned char *in, long long in_stride, unsigned char *out, long long out_stride,
	int width, int height, int bands, int es, unsigned long long alpha)
{
	if ((long long) width * (bands + 1) * es >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	const int bx = (width + FLATTEN_THREADS - 1) / FLATTEN_THREADS;
	dim3 grid(bx, pointwise_rows_grid(bx, height), 1), block(FLATTEN_THREADS, 1, 1);
	Gate gate("addalpha");
	switch (es) {
	case 1: hipLaunchKernelGGL((addalpha_kernel<unsigned char>), grid, block, 0, stream(), in, in_stride, out, out_stride, width, height, bands, alpha); break;
	case 2: hipLaunchKernelGGL((addalpha_kernel<unsigned short>), grid, block, 0, stream(), in, in_stride, out, out_stride, width, height, bands, alpha); break;
	case 4: hipLaunchKernelGGL((addalpha_kernel<unsigned int>), grid, block, 0, stream(), in, in_stride, out, out_stride, width, height, bands, alpha); break;
	case 8: hipLaunchKernelGGL((addalpha_kernel<unsigned long long>), grid, block, 0, stream(), in, in_stride, out, out_stride, width, height, bands, alpha); break;
	default:
		error(domain, "bad element size %d", es);
		return -1;
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

} // namespace vh
