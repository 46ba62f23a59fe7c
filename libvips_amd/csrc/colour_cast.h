// Part of colour.hip, which includes it: vips_cast for gfx950 (conversion/cast.c:120-330) with vips_extract_band and
// vips_bandjoin folded in, ONE kernel per region -- the kernels, their launcher and the C ABI.
#pragma once

#include "colour.h"
#include "colour_rows.h"
#include "kernel_stmt.h"

#include <climits>
#include <type_traits>

namespace vh {

template <typename TIN, typename TOUT>
struct CastOne;

// CAST_INT_INT: through int (<= 16 bit targets) or int64 (32 bit targets)
#define CAST_II(TIN, TOUT, TEMP, LO, HI) \
	template <> \
	struct CastOne<TIN, TOUT> { \
		static __device__ __forceinline__ TOUT run(TIN v) \
		{ \
			TEMP t = (TEMP) v; \
			t = t > (TEMP) (HI) ? (TEMP) (HI) : t; \
			t = t < (TEMP) (LO) ? (TEMP) (LO) : t; \
			return (TOUT) t; \
		} \
	};
#define CAST_II_ALL(TIN) \
	CAST_II(TIN, unsigned char, int, 0, UCHAR_MAX) \
	CAST_II(TIN, signed char, int, SCHAR_MIN, SCHAR_MAX) \
	CAST_II(TIN, unsigned short, int, 0, USHRT_MAX) \
	CAST_II(TIN, short, int, SHRT_MIN, SHRT_MAX) \
	CAST_II(TIN, unsigned int, long long, 0, UINT_MAX) \
	CAST_II(TIN, int, long long, INT_MIN, INT_MAX)
CAST_II_ALL(unsigned char)
CAST_II_ALL(signed char)
CAST_II_ALL(unsigned short)
CAST_II_ALL(short)
CAST_II_ALL(unsigned int)
CAST_II_ALL(int)
#undef CAST_II_ALL
#undef CAST_II

// CAST_FLOAT_INT: clip as double, then C truncation
#define CAST_FI(TIN, TOUT, LO, HI) \
	template <> \
	struct CastOne<TIN, TOUT> { \
		static __device__ __forceinline__ TOUT run(TIN v) \
		{ \
			double d = (double) v; \
			d = (double) (HI) < d ? (double) (HI) : d; \
			d = (double) (LO) > d ? (double) (LO) : d; \
			return vh::cvt_to<TOUT>(d); \
		} \
	};
#define CAST_FI_ALL(TIN) \
	CAST_FI(TIN, unsigned char, 0, UCHAR_MAX) \
	CAST_FI(TIN, signed char, SCHAR_MIN, SCHAR_MAX) \
	CAST_FI(TIN, unsigned short, 0, USHRT_MAX) \
	CAST_FI(TIN, short, SHRT_MIN, SHRT_MAX) \
	CAST_FI(TIN, unsigned int, 0, UINT_MAX) \
	CAST_FI(TIN, int, INT_MIN, INT_MAX)
CAST_FI_ALL(float)
CAST_FI_ALL(double)
#undef CAST_FI_ALL
#undef CAST_FI

// CAST_REAL_FLOAT: plain conversion
#define CAST_RF(TIN, TOUT) \
	template <> \
	struct CastOne<TIN, TOUT> { \
		static __device__ __forceinline__ TOUT run(TIN v) { return (TOUT) v; } \
	};
#define CAST_RF_ALL(TIN) \
	CAST_RF(TIN, float) \
	CAST_RF(TIN, double)
CAST_RF_ALL(unsigned char)
CAST_RF_ALL(signed char)
CAST_RF_ALL(unsigned short)
CAST_RF_ALL(short)
CAST_RF_ALL(unsigned int)
CAST_RF_ALL(int)
CAST_RF_ALL(float)
CAST_RF_ALL(double)
#undef CAST_RF_ALL
#undef CAST_RF

struct CastArgs {
	const unsigned char *in;
	unsigned char *out;
	long long in_stride, out_stride;
	int ne; // elements per row copied
	int height;
	// band remap for extract_band / bandjoin: element e of the output row reads
	// input pel e / out_take, band in_first + e % out_take; writes band out_first + ...
	int in_bands, out_bands, in_first, out_first, take;
};

template <typename TIN, typename TOUT>
__global__ void __launch_bounds__(256)
cast_kernel(CastArgs a)
{
	const int e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= a.ne)
		return;
	const int x = e / a.take;
	const int b = e - x * a.take;
	const long long ie = (long long) x * a.in_bands + a.in_first + b;
	const long long oe = (long long) x * a.out_bands + a.out_first + b;
	for (int y0 = blockIdx.y * RU; y0 < a.height; y0 += gridDim.y * RU) {
		TIN v[RU];
#pragma unroll
		for (int r = 0; r < RU; r++) {
			const int y = min(y0 + r, a.height - 1);
			v[r] = ((const TIN *) (a.in + (long long) y * a.in_stride))[ie];
		}
#pragma unroll
		for (int r = 0; r < RU; r++)
			if (y0 + r < a.height)
				((TOUT *) (a.out + (long long) (y0 + r) * a.out_stride))[oe] = CastOne<TIN, TOUT>::run(v[r]);
	}
}

// A plain cast (every band, rows that start where a group of four elements does on both sides): a lane owns FOUR
// neighbouring elements -- one load, one store of 4 x sizeof (16 bytes for a float: a wave writes 1 KiB of a line
// in one instruction) -- and RU rows are in flight per lane.  vips_cast's arithmetic is CastOne's, element by
// element (conversion/cast.c:120-330); round 5's one-element-per-lane form ran at 56 % of 8 TB/s on uchar -> float.
template <typename T>
struct alignas(4 * sizeof(T)) CastQuad {
	T v[4];
};

template <typename TIN, typename TOUT>
__global__ void __launch_bounds__(256)
cast_quad_kernel(CastArgs a)
{
	const int g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= a.ne / 4)
		return;
	for (int y0 = blockIdx.y * RU; y0 < a.height; y0 += gridDim.y * RU) {
		CastQuad<TIN> v[RU];
#pragma unroll
		for (int r = 0; r < RU; r++) {
			const int y = min(y0 + r, a.height - 1);
			v[r] = ((const CastQuad<TIN> *) (a.in + (long long) y * a.in_stride))[g];
		}
#pragma unroll
		for (int r = 0; r < RU; r++)
			if (y0 + r < a.height) {
				CastQuad<TOUT> o;
#pragma unroll
				for (int i = 0; i < 4; i++)
					o.v[i] = CastOne<TIN, TOUT>::run(v[r].v[i]);
				((CastQuad<TOUT> *) (a.out + (long long) (y0 + r) * a.out_stride))[g] = o;
			}
	}
}

template <typename TIN, typename TOUT>
static bool cast_quad_ok(const CastArgs &a)
{
	if (a.take != a.in_bands || a.take != a.out_bands || a.in_first != 0 || a.out_first != 0 || a.ne < 1024)
		return false;
	if (getenv("VIPS_HIP_NO_CAST_QUAD"))
		return false;
	return !(((uintptr_t) a.in | (uintptr_t) a.in_stride) % (4 * sizeof(TIN))) &&
		!(((uintptr_t) a.out | (uintptr_t) a.out_stride) % (4 * sizeof(TOUT)));
}

template <typename TIN>
static int launch_cast_out(const CastArgs &a_all, int out_format)
{
	dim3 block(256, 1, 1);
	CastArgs a = a_all;
	Gate gate("cast");
#define GO(TOUT) \
	if (cast_quad_ok<TIN, TOUT>(a)) { \
		const int groups = a.ne / 4; \
		dim3 qgrid((groups + 255) / 256, rows_grid((groups + 255) / 256, a.height), 1); \
		hipLaunchKernelGGL((cast_quad_kernel<TIN, TOUT>), qgrid, block, 0, stream(), a); \
		/* the last ne % 4 elements of every row: the element kernel on what is left */ \
		a.in += (size_t) groups * 4 * sizeof(TIN); \
		a.out += (size_t) groups * 4 * sizeof(TOUT); \
		a.ne -= groups * 4; \
		/* (a.take stays: x = e / take, b = e % take address the same elements from the moved base \
		   only when the split falls on a pixel boundary or take == bands == the whole row's period; \
		   with every band taken ie == oe == e, so any split is right) */ \
	} \
	if (a.ne > 0) { \
		dim3 grid((a.ne + 255) / 256, rows_grid((a.ne + 255) / 256, a.height), 1); \
		hipLaunchKernelGGL((cast_kernel<TIN, TOUT>), grid, block, 0, stream(), a); \
	} \
	break;
	switch (out_format) {
	case VIPS_HIP_FORMAT_UCHAR: GO(unsigned char)
	case VIPS_HIP_FORMAT_CHAR: GO(signed char)
	case VIPS_HIP_FORMAT_USHORT: GO(unsigned short)
	case VIPS_HIP_FORMAT_SHORT: GO(short)
	case VIPS_HIP_FORMAT_UINT: GO(unsigned int)
	case VIPS_HIP_FORMAT_INT: GO(int)
	case VIPS_HIP_FORMAT_FLOAT: GO(float)
	case VIPS_HIP_FORMAT_DOUBLE: GO(double)
	default:
		error("cast", "unsupported band format %d", out_format);
		return -1;
	}
#undef GO
	VH_CHECK(hipGetLastError());
	return 0;
}

int band_cast(const VipsHipRegion *in, int in_first, const VipsHipRegion *out, int out_first, int take)
{
	if (ensure_init())
		return -1;
	if (check_region("cast", in) || check_region("cast", out))
		return -1;
	if (format_iscomplex(in->format) || format_iscomplex(out->format)) {
		error("cast", "complex formats are outside the HIP path");
		return -1;
	}
	if (out->left < in->left || out->top < in->top ||
		out->left + out->width > in->left + in->width ||
		out->top + out->height > in->top + in->height) {
		error("cast", "input region too small");
		return -1;
	}
	if (in_first < 0 || take <= 0 || in_first + take > in->bands || out_first < 0 ||
		out_first + take > out->bands) {
		error("cast", "bad band range");
		return -1;
	}
	CastArgs a;
	const int ies = format_sizeof(in->format);
	a.in = (const unsigned char *) in->data + (size_t) (out->top - in->top) * in->stride +
		(size_t) (out->left - in->left) * in->bands * ies;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) out->stride;
	a.ne = out->width * take;
	a.height = out->height;
	a.in_bands = in->bands;
	a.out_bands = out->bands;
	a.in_first = in_first;
	a.out_first = out_first;
	a.take = take;
	switch (in->format) {
	case VIPS_HIP_FORMAT_UCHAR: return launch_cast_out<unsigned char>(a, out->format);
	case VIPS_HIP_FORMAT_CHAR: return launch_cast_out<signed char>(a, out->format);
	case VIPS_HIP_FORMAT_USHORT: return launch_cast_out<unsigned short>(a, out->format);
	case VIPS_HIP_FORMAT_SHORT: return launch_cast_out<short>(a, out->format);
	case VIPS_HIP_FORMAT_UINT: return launch_cast_out<unsigned int>(a, out->format);
	case VIPS_HIP_FORMAT_INT: return launch_cast_out<int>(a, out->format);
	case VIPS_HIP_FORMAT_FLOAT: return launch_cast_out<float>(a, out->format);
	case VIPS_HIP_FORMAT_DOUBLE: return launch_cast_out<double>(a, out->format);
	default:
		error("cast", "unsupported band format %d", in->format);
		return -1;
	}
}

} // namespace vh

using namespace vh;

extern "C" {

int vips_hip_cast_gen(const VipsHipRegion *in, const VipsHipRegion *out)
{
	if (in && out && in->bands != out->bands) {
		error("cast", "input and output must have the same number of bands");
		return -1;
	}
	return band_cast(in, 0, out, 0, in ? in->bands : 0);
}

} // extern "C"
