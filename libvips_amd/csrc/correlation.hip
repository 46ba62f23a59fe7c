// vips_fastcor and vips_spcor (convolution/fastcor.c, spcor.c, correlation.c) for gfx950: a reference image slid over
// an image, one number an output element.  Output element (x, y, b) compares band b of the ref with the window of the
// embedded image whose top-left corner is (x, y): the image sits at (ref_w / 2, ref_h / 2) of a canvas of
// in.size + ref.size - 1 whose edges are copies (correlation.c:91-96).  The canvas is never made: the clamp is in the
// loads that stage a block's tile.
//
// Shape.  The cost is arithmetic, ref_w * ref_h taps an element, and every tap of the float and the spcor sums is a
// rounded operation whose order is the reference's (rows of the ref, then columns): one output element is one serial
// chain, and a lane owns COR_R of them.  A block of 256 lanes makes COR_TW x COR_TH = 32 x 32 pels of ONE band
// (blockIdx.z): its LDS holds that band of the halo tile -- (32 + ref_w - 1) x (32 + ref_h - 1) elements in the image's
// own type, loaded element by element with the pel clamped to the image -- and that band of the ref: its elements for
// fastcor, for spcor the doubles (rp - rmean[b]) the host has tabulated.  A lane's COR_R outputs are COR_R rows of one
// column, COR_TH / COR_R rows apart: a tap reads the ref once (every lane the same address: a broadcast) and the tile
// COR_R times (a wave reads two runs of 32 consecutive elements).
//
//   fastcor_<type>   integers: sum += (unsigned) t * t, t = ref - in, modulo 2^32 in any order; float and double:
//                    sum = sum + dif * dif in the type, unfused.
//   spcor_<type>     sum1 over the window and imean = sum1 / N, then t = ip - imean, sum2 += t * t,
//                    sum3 += (rp - rmean[b]) * t, all double and unfused, in raster order; c2 = c1[b] * sqrt(sum2);
//                    +0 where c2 == 0, else sum3 / c2, as a float.
#include "gcn.h"
#include "internal.h"
#include "pointwise.h"

namespace vh {

constexpr int COR_THREADS = 256;
constexpr int COR_TW = 32, COR_TH = 32; // pels of a block's tile
constexpr int COR_R = 4;                // outputs a lane
constexpr int COR_LANE_ROWS = COR_THREADS / COR_TW; // rows the block's lanes span: a lane's outputs are this far apart
constexpr int COR_MAX_SIDE = VIPS_HIP_CORRELATION_MAX_SIDE;
constexpr int COR_LDS_MAX = 160 * 1024; // a CU's LDS
static_assert(COR_LANE_ROWS * COR_R == COR_TH, "a block's lanes cover its tile");

// the bytes of the tile, rounded up to where the ref's table starts
static inline __host__ __device__ int cor_tile_bytes(int ref_w, int ref_h, int es)
{
	return ((COR_TW + ref_w - 1) * (COR_TH + ref_h - 1) * es + 7) & ~7;
}

// band `band` of the halo tile whose output corner is (x0, y0), and that band of the ref to `tab`: its elements, or
// (SPCOR) the host's table
template <typename T, bool SPCOR>
VH_DEV void cor_stage(const CorrelationArgs &a, T *tile, typename std::conditional<SPCOR, double, T>::type *tab, int x0, int y0, int band)
{
	const int tile_w = COR_TW + a.ref_w - 1, tile_h = COR_TH + a.ref_h - 1;
	const int ib = a.in_bands == 1 ? 0 : band;
	const int lane = tid() & 63, wave = tid() >> 6;
	for (int r = wave; r < tile_h; r += COR_THREADS / 64) {
		int y = y0 + r - a.ref_h / 2;
		y = y < 0 ? 0 : y > a.height - 1 ? a.height - 1 : y;
		const T *row = (const T *) (a.in + (long long) y * a.in_stride);
		for (int c = lane; c < tile_w; c += 64) {
			int x = x0 + c - a.ref_w / 2;
			x = x < 0 ? 0 : x > a.width - 1 ? a.width - 1 : x;
			tile[r * tile_w + c] = row[x * a.in_bands + ib];
		}
	}
	if constexpr (SPCOR) {
		// spcor: the host's table, band-major
		const double *src = a.table + (long long) band * a.ref_w * a.ref_h;
		for (int i = tid(); i < a.ref_w * a.ref_h; i += COR_THREADS)
			tab[i] = src[i];
	}
	else {
		const int rb = a.ref_bands == 1 ? 0 : band;
		for (int i = tid(); i < a.ref_w * a.ref_h; i += COR_THREADS) {
			const int j = i / a.ref_w;
			tab[i] = ((const T *) (a.ref + (long long) j * a.ref_stride))[(i - j * a.ref_w) * a.ref_bands + rb];
		}
	}
}

// a lane's outputs: column x, rows y + k * COR_LANE_ROWS; tile element (0, 0) of output k's window is at[k]
struct CorLane {
	int x, y;
	int at[COR_R];
};
VH_DEV CorLane cor_lane(const CorrelationArgs &a)
{
	CorLane l;
	const int tx = tid() % COR_TW, ty = tid() / COR_TW;
	l.x = (int) blockIdx.x * COR_TW + tx;
	l.y = (int) blockIdx.y * COR_TH + ty;
#pragma unroll
	for (int k = 0; k < COR_R; k++)
		l.at[k] = (ty + k * COR_LANE_ROWS) * (COR_TW + a.ref_w - 1) + tx;
	return l;
}

template <typename OUT>
VH_DEV void cor_store(const CorrelationArgs &a, const CorLane &l, int band, const OUT (&v)[COR_R])
{
	if (l.x >= a.width)
		return;
#pragma unroll
	for (int k = 0; k < COR_R; k++) {
		const int y = l.y + k * COR_LANE_ROWS;
		if (y < a.height)
			((OUT *) (a.out + (long long) y * a.out_stride))[l.x * a.bands + band] = v[k];
	}
}

template <typename T>
struct FastcorSum {
	typedef unsigned int type;
};
template <>
struct FastcorSum<float> {
	typedef float type;
};
template <>
struct FastcorSum<double> {
	typedef double type;
};

// fastcor.c:74-134
template <typename T>
__global__ void __launch_bounds__(COR_THREADS)
fastcor_kernel(CorrelationArgs a)
{
	typedef typename FastcorSum<T>::type S;
	VH_DYNAMIC_LDS(unsigned char, lds);
	T *tile = (T *) lds;
	T *tab = (T *) (lds + cor_tile_bytes(a.ref_w, a.ref_h, (int) sizeof(T)));
	const int band = (int) blockIdx.z;
	cor_stage<T, false>(a, tile, tab, (int) blockIdx.x * COR_TW, (int) blockIdx.y * COR_TH, band);
	barrier();

	const CorLane l = cor_lane(a);
	const int tile_w = COR_TW + a.ref_w - 1;
	S sum[COR_R];
#pragma unroll
	for (int k = 0; k < COR_R; k++)
		sum[k] = (S) 0;
	for (int j = 0; j < a.ref_h; j++) {
		const T *rrow = tab + j * a.ref_w;
		for (int i = 0; i < a.ref_w; i++) {
			const T r = rrow[i];
#pragma unroll
			for (int k = 0; k < COR_R; k++) {
				const T p = tile[l.at[k] + j * tile_w + i];
				if constexpr (std::is_same<T, float>::value) {
					const float dif = __fsub_rn(r, p);
					sum[k] = __fadd_rn(sum[k], __fmul_rn(dif, dif));
				}
				else if constexpr (std::is_same<T, double>::value) {
					const double dif = __dsub_rn(r, p);
					sum[k] = __dadd_rn(sum[k], __dmul_rn(dif, dif));
				}
				else {
					// int t = ref - in; sum += (unsigned int) t * t: everything modulo 2^32
					const unsigned int t = (unsigned int) (int) r - (unsigned int) (int) p;
					sum[k] += t * t;
				}
			}
		}
	}
	cor_store<S>(a, l, band, sum);
}

// spcor.c:154-290
template <typename T>
__global__ void __launch_bounds__(COR_THREADS)
spcor_kernel(CorrelationArgs a)
{
	VH_DYNAMIC_LDS(unsigned char, lds);
	T *tile = (T *) lds;
	double *tab = (double *) (lds + cor_tile_bytes(a.ref_w, a.ref_h, (int) sizeof(T)));
	const int band = (int) blockIdx.z;
	cor_stage<T, true>(a, tile, tab, (int) blockIdx.x * COR_TW, (int) blockIdx.y * COR_TH, band);
	barrier();

	const CorLane l = cor_lane(a);
	const int tile_w = COR_TW + a.ref_w - 1;
	const double n = (double) (a.ref_w * a.ref_h);
	double imean[COR_R], sum2[COR_R], sum3[COR_R];
#pragma unroll
	for (int k = 0; k < COR_R; k++)
		imean[k] = sum2[k] = sum3[k] = 0.0;
	// the mean of the window
	for (int j = 0; j < a.ref_h; j++)
		for (int i = 0; i < a.ref_w; i++) {
#pragma unroll
			for (int k = 0; k < COR_R; k++)
				imean[k] = __dadd_rn(imean[k], (double) tile[l.at[k] + j * tile_w + i]);
		}
#pragma unroll
	for (int k = 0; k < COR_R; k++)
		imean[k] = __ddiv_rn(imean[k], n);
	for (int j = 0; j < a.ref_h; j++) {
		const double *rrow = tab + j * a.ref_w;
		for (int i = 0; i < a.ref_w; i++) {
			const double rd = rrow[i];
#pragma unroll
			for (int k = 0; k < COR_R; k++) {
				const double t = __dsub_rn((double) tile[l.at[k] + j * tile_w + i], imean[k]);
				sum2[k] = __dadd_rn(sum2[k], __dmul_rn(t, t));
				sum3[k] = __dadd_rn(sum3[k], __dmul_rn(rd, t));
			}
		}
	}
	const double c1 = a.c1[band];
	float cc[COR_R];
#pragma unroll
	for (int k = 0; k < COR_R; k++) {
		const double c2 = __dmul_rn(c1, sqrt(sum2[k]));
		// (something like a constant ref, or a constant window: uncorrelated)
		cc[k] = c2 == 0.0 ? 0.0f : (float) __ddiv_rn(sum3[k], c2);
	}
	cor_store<float>(a, l, band, cc);
}

template <typename T>
static int cor_launch(const char *domain, const CorrelationArgs &a, int spcor, const char *gate_name)
{
	const long long lds = cor_tile_bytes(a.ref_w, a.ref_h, (int) sizeof(T)) + (long long) a.ref_w * a.ref_h * (spcor ? 8 : (int) sizeof(T));
	if (lds > COR_LDS_MAX) {
		error(domain, "a %d x %d ref needs %lld KB of LDS, the kernel has %d", a.ref_w, a.ref_h, (lds + 1023) / 1024, COR_LDS_MAX / 1024);
		return -1;
	}
	const auto kernel = spcor ? spcor_kernel<T> : fastcor_kernel<T>;
	if (lds > 64 * 1024)
		VH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, COR_LDS_MAX));
	const dim3 grid((unsigned int) ((a.width + COR_TW - 1) / COR_TW), (unsigned int) ((a.height + COR_TH - 1) / COR_TH), (unsigned int) a.bands);
	{
		Gate gate(gate_name);
		hipLaunchKernelGGL(kernel, grid, dim3(COR_THREADS), (size_t) lds, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

// Everything has been checked (ops_correlation.cpp).
int correlation_run(const char *domain, CorrelationArgs a, int format, int spcor)
{
	if (a.ref_w < 1 || a.ref_h < 1 || a.ref_w > COR_MAX_SIDE || a.ref_h > COR_MAX_SIDE) {
		error(domain, "a %d x %d ref: the kernel takes refs up to %d x %d", a.ref_w, a.ref_h, COR_MAX_SIDE, COR_MAX_SIDE);
		return -1;
	}
	if (a.width < 1 || a.height < 1 || a.bands < 1 || a.bands > 65535 || (long long) a.width * a.bands >= (1LL << 31) ||
		(long long) (a.height + COR_TH - 1) / COR_TH > 65535) {
		error(domain, "image too large");
		return -1;
	}
	const uintptr_t es = (uintptr_t) format_sizeof(format);
	if (es == 0 || format_iscomplex(format)) {
		error(domain, "no kernel for format %d", format);
		return -1;
	}
	if (((uintptr_t) a.in | (uintptr_t) a.in_stride | (uintptr_t) a.ref | (uintptr_t) a.ref_stride) % es ||
		((uintptr_t) a.out | (uintptr_t) a.out_stride) % (spcor || es < 4 ? 4 : es)) {
		error(domain, "rows must start on whole elements");
		return -1;
	}
	static const char *const fast_gates[] = { "fastcor_u8", "fastcor_s8", "fastcor_u16", "fastcor_s16", "fastcor_u32", "fastcor_s32", "fastcor_f32",
		nullptr, "fastcor_f64" };
	static const char *const sp_gates[] = { "spcor_u8", "spcor_s8", "spcor_u16", "spcor_s16", "spcor_u32", "spcor_s32", "spcor_f32", nullptr,
		"spcor_f64" };
	const char *gate = (spcor ? sp_gates : fast_gates)[format];
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR: return cor_launch<u8>(domain, a, spcor, gate);
	case VIPS_HIP_FORMAT_CHAR: return cor_launch<s8>(domain, a, spcor, gate);
	case VIPS_HIP_FORMAT_USHORT: return cor_launch<u16>(domain, a, spcor, gate);
	case VIPS_HIP_FORMAT_SHORT: return cor_launch<s16>(domain, a, spcor, gate);
	case VIPS_HIP_FORMAT_UINT: return cor_launch<u32>(domain, a, spcor, gate);
	case VIPS_HIP_FORMAT_INT: return cor_launch<s32>(domain, a, spcor, gate);
	case VIPS_HIP_FORMAT_FLOAT: return cor_launch<f32>(domain, a, spcor, gate);
	default: return cor_launch<f64>(domain, a, spcor, gate);
	}
}

int correlation_tile(int what)
{
	return what == 0 ? COR_TW : what == 1 ? COR_TH : what == 2 ? COR_MAX_SIDE : 0;
}

} // namespace vh
