// vips_recomb (conversion/recomb.c:75-205) on the device (gfx950): out[v] = (OUT) sum_u m[v][u] * in[u], an
// mheight-band pel from an mwidth-band pel, ONE launch.
//
// The arithmetic is the reference's LOOP (recomb.c:75-98), statement by statement: t starts at 0.0 and takes the
// products in order u = 0 .. mwidth - 1, in double, a multiply and an add each (__dmul_rn / __dadd_rn: the reference is
// baseline x86-64 code, which has no fused multiply-add); the store is the conversion of the double to float (double for
// a double image), which rounds to nearest and overflows to an infinity.  The leading 0.0 + is kept: it turns a first
// product of -0.0 into +0.0.
//
//   recomb_stream<IN, MW, MH>   the band counts pipelines use (3 -> 3, 3 -> 1, 1 -> 3, 4 -> 4, 4 -> 3, 3 -> 4) on uchar,
//                               ushort and float, known when the kernel is compiled: the coefficients are read from the
//                               kernel's arguments with constant indices and stay in scalar registers.  A lane takes a
//                               RUN of pels, the smallest whose input is whole dwords and whose output (floats) is whole
//                               16-byte groups -- four RGB uchar pels are three dwords in and three global_store_dwordx4
//                               out -- with rows that start on dwords on both sides.  The runs of every row are dealt to
//                               the lanes as one sequence; rows that follow one another without a gap are one row
//                               (as pointwise.h joins them), and a ragged last run goes pel by pel in the same launch.
//   recomb_general<IN, OUT>     one output pel a lane, the matrix in LDS, mwidth and mheight at run time: any format, any
//                               shape up to 32 x 32, rows that start on any element.  It defines correctness;
//                               VIPS_HIP_NO_RECOMB_STREAM sends everything to it.
#include "pointwise.h"

namespace vh {

constexpr int RECOMB_THREADS = POINTWISE_THREADS;

// pels of a run: the fewest whose `mw` elements of `es` bytes are whole dwords and whose `mh` floats are whole 16-byte
// groups (four always are)
constexpr int recomb_run_pels(int es, int mw, int mh)
{
	for (int p = 1; p < 4; p++)
		if (p * mw * es % 4 == 0 && p * mh % 4 == 0)
			return p;
	return 4;
}

// `ND` dwords at a dword-aligned offset: 16 bytes at a time, then what is left
template <int ND>
VH_DEV void recomb_load(gptr_in base, unsigned int off, unsigned int (&d)[ND])
{
#pragma unroll
	for (int q = 0; q < ND / 4; q++) {
		unsigned int t[4];
		gload128(base, off + 16u * (unsigned int) q, t);
#pragma unroll
		for (int i = 0; i < 4; i++)
			d[4 * q + i] = t[i];
	}
	if constexpr (ND % 4 != 0) {
		unsigned int t[ND % 4];
		gload_dwords<ND % 4>(base, off + 16u * (unsigned int) (ND / 4), t);
#pragma unroll
		for (int i = 0; i < ND % 4; i++)
			d[ND / 4 * 4 + i] = t[i];
	}
}

template <typename IN, int MW, int MH>
__global__ void __launch_bounds__(RECOMB_THREADS)
recomb_stream_kernel(RecombArgs a)
{
	constexpr int P = recomb_run_pels((int) sizeof(IN), MW, MH);
	constexpr int ND = P * MW * (int) sizeof(IN) / 4; // dwords of a run's input
	constexpr int NQ = P * MH / 4;                    // 16-byte groups of its output
	const unsigned int total = (unsigned int) a.runs * (unsigned int) a.height;
	for (unsigned int at = (unsigned int) blockIdx.x * RECOMB_THREADS + (unsigned int) threadIdx.x; at < total; at += (unsigned int) gridDim.x * RECOMB_THREADS) {
		const int y = (int) (at / (unsigned int) a.runs);
		const int r = (int) (at - (unsigned int) y * (unsigned int) a.runs);
		const int p0 = r * P;
		const int n = min(P, a.width - p0); // < P: the row's ragged end
		const unsigned long long irow = (unsigned long long) a.in + (unsigned long long) y * a.in_stride;
		const unsigned long long orow = (unsigned long long) a.out + (unsigned long long) y * a.out_stride;
		if (n == P) {
			unsigned int d[ND], w[NQ * 4];
			recomb_load<ND>(gptr_in_of(irow), (unsigned int) r * (unsigned int) (ND * 4), d);
#pragma unroll
			for (int i = 0; i < P; i++) {
#pragma unroll
				for (int v = 0; v < MH; v++) {
					double t = 0.0;
#pragma unroll
					for (int u = 0; u < MW; u++) {
						const IN p = group_take<IN, ND>(d, i * MW + u);
						t = __dadd_rn(t, __dmul_rn(a.m[v * MW + u], (double) p));
					}
					w[i * MH + v] = __builtin_bit_cast(unsigned int, (float) t);
				}
			}
#pragma unroll
			for (int q = 0; q < NQ; q++) {
				const unsigned int g[4] = { w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3] };
				gstore128(gptr_out_of(orow) + (unsigned int) r * (unsigned int) (NQ * 16) + 16u * (unsigned int) q, g);
			}
		}
		else {
			for (int i = 0; i < n; i++) {
				const IN *p = (const IN *) irow + (long long) (p0 + i) * MW;
				float *q = (float *) orow + (long long) (p0 + i) * MH;
#pragma unroll
				for (int v = 0; v < MH; v++) {
					double t = 0.0;
#pragma unroll
					for (int u = 0; u < MW; u++)
						t = __dadd_rn(t, __dmul_rn(a.m[v * MW + u], (double) p[u]));
					q[v] = (float) t;
				}
			}
		}
	}
}

template <typename IN, typename OUT>
__global__ void __launch_bounds__(RECOMB_THREADS)
recomb_general_kernel(RecombArgs a)
{
	__shared__ double m[RECOMB_MAX * RECOMB_MAX];
	for (int i = tid(); i < a.mwidth * a.mheight; i += RECOMB_THREADS)
		m[i] = a.matrix[i];
	barrier();
	const int x = (int) blockIdx.x * RECOMB_THREADS + tid();
	if (x >= a.width)
		return;
	for (int y = (int) blockIdx.y; y < a.height; y += (int) gridDim.y) {
		const IN *p = (const IN *) (a.in + (long long) y * a.in_stride) + (long long) x * a.mwidth;
		OUT *q = (OUT *) (a.out + (long long) y * a.out_stride) + (long long) x * a.mheight;
		for (int v = 0; v < a.mheight; v++) {
			double t = 0.0;
			for (int u = 0; u < a.mwidth; u++)
				t = __dadd_rn(t, __dmul_rn(m[v * a.mwidth + u], (double) p[u]));
			q[v] = (OUT) t;
		}
	}
}

// ---------------------------------------------------------------- dispatch

static bool recomb_stream_shape(int mw, int mh)
{
	return (mw == 3 && (mh == 3 || mh == 1 || mh == 4)) || (mw == 1 && mh == 3) || (mw == 4 && (mh == 4 || mh == 3));
}

// The stream kernel takes this call: then its rows are joined and `runs` is set.
static bool recomb_streams(RecombArgs &a, int format)
{
	if (getenv("VIPS_HIP_NO_RECOMB_STREAM") || !recomb_stream_shape(a.mwidth, a.mheight))
		return false;
	if (format != VIPS_HIP_FORMAT_UCHAR && format != VIPS_HIP_FORMAT_USHORT && format != VIPS_HIP_FORMAT_FLOAT)
		return false;
	const int es = format_sizeof(format);
	const long long in_pel = (long long) a.mwidth * es, out_pel = (long long) a.mheight * (long long) sizeof(float);
	RecombArgs joined = a;
	// (one row is nothing away from a next one: its stride must not count in the alignment)
	if (joined.height == 1)
		joined.in_stride = joined.out_stride = 0;
	// rows that follow one another without a gap on both sides are one long row
	if (joined.height > 1 && joined.in_stride == joined.width * in_pel && joined.out_stride == joined.width * out_pel &&
		(long long) joined.width * joined.height * (in_pel > out_pel ? in_pel : out_pel) < (1LL << 31)) {
		joined.width *= joined.height;
		joined.height = 1;
		joined.in_stride = joined.out_stride = 0;
	}
	const int p = recomb_run_pels(es, a.mwidth, a.mheight);
	const long long runs = ((long long) joined.width + p - 1) / p;
	// rows that start on dwords on both sides; the kernel numbers the runs in 32 bits
	if (!on_unit(joined.in, joined.in_stride, 4) || !on_unit(joined.out, joined.out_stride, 4) || runs * joined.height >= (1LL << 31))
		return false;
	a = joined;
	a.runs = (int) runs;
	return true;
}

template <typename IN>
static bool recomb_stream_launch(const RecombArgs &a)
{
	const dim3 grid = pointwise_stream_grid((long long) a.runs * a.height), block(RECOMB_THREADS, 1, 1);
#define SHAPE(MW, MH) \
	if (a.mwidth == MW && a.mheight == MH) { \
		hipLaunchKernelGGL((recomb_stream_kernel<IN, MW, MH>), grid, block, 0, stream(), a); \
		return true; \
	}
	SHAPE(3, 3) SHAPE(3, 1) SHAPE(1, 3) SHAPE(4, 4) SHAPE(4, 3) SHAPE(3, 4)
#undef SHAPE
	return false;
}

template <typename IN, typename OUT>
static void recomb_general_launch(const RecombArgs &a)
{
	const int bx = (a.width + RECOMB_THREADS - 1) / RECOMB_THREADS;
	dim3 grid(bx, pointwise_rows_grid(bx, a.height), 1), block(RECOMB_THREADS, 1, 1);
	hipLaunchKernelGGL((recomb_general_kernel<IN, OUT>), grid, block, 0, stream(), a);
}

int recomb_tile(int what)
{
	switch (what) {
	case 0: return RECOMB_THREADS;
	case 1: return POINTWISE_GRID_BLOCKS;
	case 2: return 4;
	default: return 0;
	}
}

// Everything has been checked (ops_recomb.cpp); `matrix`: mheight x mwidth doubles in host memory.
int recomb_run(const char *domain, int format, RecombArgs a, const double *matrix)
{
	if (a.width < 1 || a.height < 1 || a.mwidth < 1 || a.mheight < 1 || a.mwidth > RECOMB_MAX || a.mheight > RECOMB_MAX) {
		error(domain, "bad image or matrix size");
		return -1;
	}
	const int es = format_sizeof(format), out_es = format == VIPS_HIP_FORMAT_DOUBLE ? 8 : 4;
	if ((long long) a.width * a.mwidth * es >= (1LL << 31) || (long long) a.width * a.mheight * out_es >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	if (!on_unit(a.in, a.in_stride, (uintptr_t) es) || !on_unit(a.out, a.out_stride, (uintptr_t) out_es)) {
		error(domain, "rows must start on whole elements");
		return -1;
	}
	if (recomb_streams(a, format)) {
		static_assert(RECOMB_STREAM_MAX == 4, "the shapes of recomb_stream_shape");
		for (int i = 0; i < a.mwidth * a.mheight; i++)
			a.m[i] = matrix[i];
		Gate gate("recomb_stream");
		const bool launched = format == VIPS_HIP_FORMAT_UCHAR ? recomb_stream_launch<u8>(a)
			: format == VIPS_HIP_FORMAT_USHORT                ? recomb_stream_launch<u16>(a)
															  : recomb_stream_launch<f32>(a);
		if (!launched) {
			error(domain, "no stream kernel for a %d x %d matrix", a.mwidth, a.mheight);
			return -1;
		}
		VH_CHECK(hipGetLastError());
		return 0;
	}
	// (the block goes back to the pool behind the kernel: the pool hands it out again on this thread's stream only)
	const size_t bytes = (size_t) a.mwidth * a.mheight * sizeof(double);
	DeviceBlock block(bytes);
	if (!block.p || vips_hip_memcpy_h2d(block.p, matrix, bytes))
		return -1;
	a.matrix = (const double *) block.p;
	Gate gate("recomb_general");
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR: recomb_general_launch<u8, f32>(a); break;
	case VIPS_HIP_FORMAT_CHAR: recomb_general_launch<s8, f32>(a); break;
	case VIPS_HIP_FORMAT_USHORT: recomb_general_launch<u16, f32>(a); break;
	case VIPS_HIP_FORMAT_SHORT: recomb_general_launch<s16, f32>(a); break;
	case VIPS_HIP_FORMAT_UINT: recomb_general_launch<u32, f32>(a); break;
	case VIPS_HIP_FORMAT_INT: recomb_general_launch<s32, f32>(a); break;
	case VIPS_HIP_FORMAT_FLOAT: recomb_general_launch<f32, f32>(a); break;
	case VIPS_HIP_FORMAT_DOUBLE: recomb_general_launch<f64, f64>(a); break;
	default:
		error(domain, "no kernel for format %d", format);
		return -1;
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

} // namespace vh
