// The three interpolators of vips_affine on the device, shared by upsize.hip (the pure enlargement of vips_resize) and
// affine.hip (the general transform): one output pel from the continuous coordinate (x, y) of the embedded input.
//   nearest     resample/interpolate.c:336-352
//   bilinear    resample/interpolate.c:432-484: 12-bit fixed point for 8 / 16 bit formats, double for uint / int / float
//   bicubic     resample/bicubic.cpp:482-600, tables :620-633, arithmetic resample/templates.h:152-290: fixed point for
//               (u)char, double with clip for the 16 / 32-bit integers, double rounded to float per row for float
// All float arithmetic in the reference's order with separately rounded operations (the library is built with
// -ffp-contract=off).  How an embedded coordinate becomes a pel is the caller's: `fetch(ex, ey, band)`.
#pragma once

#include "resample.h"
#include "kernel_stmt.h"

#include <climits>
#include <type_traits>

namespace vh {

// TRANSFORM_SCALE (64), INTERPOLATE_SHIFT (12), INTERPOLATE_SCALE: resample.h

struct BicubicTables {
	int mi[TRANSFORM_SCALE + 1][4];
	double mf[TRANSFORM_SCALE + 1][4];
};
// the tables of bicubic.cpp:624-633 in the calling thread's device's memory, made once per device (upsize.hip)
const BicubicTables *bicubic_tables();

static __device__ __forceinline__ int unsigned_fixed_round(int v)
{
	return (v + (INTERPOLATE_SCALE >> 1)) >> INTERPOLATE_SHIFT;
}

static __device__ __forceinline__ int signed_fixed_round(int v)
{
	const int sign_of_v = 2 * (v >= 0) - 1;
	const int round_by = sign_of_v * (INTERPOLATE_SCALE >> 1);
	return (v + round_by) >> INTERPOLATE_SHIFT;
}

template <typename T>
struct UpTraits; // INT_PATH: fixed-point bilinear / bicubic; LO / HI: clip of the double bicubic
#define UP_TRAITS(TYPE, FIXED, SIGNED_, LO_, HI_) \
	template <> \
	struct UpTraits<TYPE> { \
		static constexpr bool fixed_bilinear = FIXED; \
		static constexpr bool is_signed = SIGNED_; \
		static __device__ __forceinline__ double lo() { return (double) (LO_); } \
		static __device__ __forceinline__ double hi() { return (double) (HI_); } \
		static constexpr int ilo = (int) (LO_); \
		static constexpr int ihi = (int) (HI_); \
	};
UP_TRAITS(unsigned char, true, false, 0, UCHAR_MAX)
UP_TRAITS(signed char, true, true, SCHAR_MIN, SCHAR_MAX)
UP_TRAITS(unsigned short, true, false, 0, USHRT_MAX)
UP_TRAITS(short, true, true, SHRT_MIN, SHRT_MAX)
UP_TRAITS(unsigned int, false, false, 0, INT_MAX)
UP_TRAITS(int, false, true, INT_MIN, INT_MAX)
UP_TRAITS(float, false, true, 0, 0)
UP_TRAITS(double, false, true, 0, 0)
#undef UP_TRAITS

// calculate_coefficients_catmull (templates.h:296-320), every operation rounded: what the
// no-table bicubic of double images evaluates per output pixel (bicubic.cpp:419-480)
static __device__ __forceinline__ void catmull_device(double c[4], const double x)
{
	const double cr1 = __dsub_rn(1.0, x);
	const double cr2 = __dmul_rn(-0.5, x);
	const double cr3 = __dmul_rn(cr1, cr2);
	const double cone = __dmul_rn(cr1, cr3);
	const double cfou = __dmul_rn(x, cr3);
	const double cr4 = __dsub_rn(cfou, cone);
	const double ctwo = __dadd_rn(__dsub_rn(cr1, cone), cr4);
	const double cthr = __dsub_rn(__dsub_rn(x, cfou), cr4);
	c[0] = cone;
	c[3] = cfou;
	c[1] = ctwo;
	c[2] = cthr;
}

// a * b + c * d + e * f + g * h, left to right, every operation rounded (cubic_float)
static __device__ __forceinline__ double dot4(double c0, double v0, double c1, double v1, double c2,
	double v2, double c3, double v3)
{
	double s = __dmul_rn(c0, v0);
	s = __dadd_rn(s, __dmul_rn(c1, v1));
	s = __dadd_rn(s, __dmul_rn(c2, v2));
	s = __dadd_rn(s, __dmul_rn(c3, v3));
	return s;
}

// The fetch of affine.hip and mapim.hip: the vips_embed both operations put in front of themselves (conversion/embed.c),
// never materialised.  Embedded (ex, ey) becomes a source pel or the fill pel: the original pixel (px, py) sits at
// (px + off, py + off), off = window_offset + 1.  A is the kernel's argument struct (AffineArgs, MapimArgs: the fields
// in, in_stride, in_left .. in_height, im_width, im_height, bands, window_offset, extend, fill).
template <typename T, typename A>
struct EmbedFetch {
	const A &a;
	__device__ __forceinline__ T operator()(int ex, int ey, int z) const
	{
		const int off = a.window_offset + 1;
		int px = ex - off, py = ey - off;
		const bool outside = (unsigned int) px >= (unsigned int) a.im_width || (unsigned int) py >= (unsigned int) a.im_height;
		if (outside) {
			switch (a.extend) {
			case VIPS_HIP_EXTEND_COPY:
				break; // (the clamp below)
			case VIPS_HIP_EXTEND_REPEAT:
				// embed.c:378-396: clock arithmetic
				px %= a.im_width;
				py %= a.im_height;
				px += px < 0 ? a.im_width : 0;
				py += py < 0 ? a.im_height : 0;
				break;
			case VIPS_HIP_EXTEND_MIRROR: {
				// embed.c:398-431: tiles of the image and its reflection, period twice the size
				const int w2 = 2 * a.im_width, h2 = 2 * a.im_height;
				px %= w2;
				py %= h2;
				px += px < 0 ? w2 : 0;
				py += py < 0 ? h2 : 0;
				px = px < a.im_width ? px : w2 - 1 - px;
				py = py < a.im_height ? py : h2 - 1 - py;
				break;
			}
			default:
				return ((const T *) a.fill)[z];
			}
		}
		px = min(max(px, 0), a.im_width - 1);
		py = min(max(py, 0), a.im_height - 1);
		// never outside the window (the host has checked that the window holds what the rect needs)
		px = min(max(px - a.in_left, 0), a.in_width - 1);
		py = min(max(py - a.in_top, 0), a.in_height - 1);
		return ((const T *) (a.in + (long long) py * a.in_stride))[(long long) px * a.bands + z];
	}
};

// One pel of `bands` elements at q from the embedded coordinate (x, y); INTERP 0 nearest, 1 bilinear, 2 bicubic.
template <typename T, int INTERP, typename F>
static __device__ __forceinline__ void interp_pel(T *q, const double x, const double y, const int bands,
	const BicubicTables *tables, const F &fetch)
{
	const int ix = vh::cvt_i32(x);
	const int iy = vh::cvt_i32(y);
	if (INTERP == 0) {
		for (int z = 0; z < bands; z++)
			q[z] = fetch(ix, iy, z);
	}
	else if (INTERP == 1) {
		if (UpTraits<T>::fixed_bilinear) {
			const int X = vh::cvt_i32(__dmul_rn(__dsub_rn(x, (double) ix), (double) INTERPOLATE_SCALE));
			const int Y = vh::cvt_i32(__dmul_rn(__dsub_rn(y, (double) iy), (double) INTERPOLATE_SCALE));
			const int Yd = INTERPOLATE_SCALE - Y;
			const int c4 = (Y * X) >> INTERPOLATE_SHIFT;
			const int c2 = (Yd * X) >> INTERPOLATE_SHIFT;
			const int c3 = Y - c4;
			const int c1 = Yd - c2;
			for (int z = 0; z < bands; z++)
				q[z] = (T) ((c1 * (int) fetch(ix, iy, z) + c2 * (int) fetch(ix + 1, iy, z) +
								c3 * (int) fetch(ix, iy + 1, z) + c4 * (int) fetch(ix + 1, iy + 1, z) +
								(1 << INTERPOLATE_SHIFT) / 2) >>
					INTERPOLATE_SHIFT);
		}
		else {
			const double X = __dsub_rn(x, (double) ix);
			const double Y = __dsub_rn(y, (double) iy);
			const double Yd = __dsub_rn(1.0, Y);
			const double c4 = __dmul_rn(Y, X);
			const double c2 = __dmul_rn(Yd, X);
			const double c3 = __dsub_rn(Y, c4);
			const double c1 = __dsub_rn(Yd, c2);
			for (int z = 0; z < bands; z++)
				q[z] = vh::cvt_to<T>(dot4(c1, (double) fetch(ix, iy, z), c2, (double) fetch(ix + 1, iy, z), c3,
					(double) fetch(ix, iy + 1, z), c4, (double) fetch(ix + 1, iy + 1, z)));
		}
	}
	else {
		// bicubic.cpp:488-502: table index with round to nearest
		const int sx = vh::cvt_i32(__dmul_rn(__dmul_rn(x, (double) TRANSFORM_SCALE), 2.0));
		const int sy = vh::cvt_i32(__dmul_rn(__dmul_rn(y, (double) TRANSFORM_SCALE), 2.0));
		const int tx = ((sx & (TRANSFORM_SCALE * 2 - 1)) + 1) >> 1;
		const int ty = ((sy & (TRANSFORM_SCALE * 2 - 1)) + 1) >> 1;
		if (sizeof(T) == 1) {
			const int *cx = tables->mi[tx];
			const int *cy = tables->mi[ty];
			for (int z = 0; z < bands; z++) {
				int r[4];
#pragma unroll
				for (int j = 0; j < 4; j++) {
					const int s = cx[0] * (int) fetch(ix - 1, iy - 1 + j, z) + cx[1] * (int) fetch(ix, iy - 1 + j, z) +
						cx[2] * (int) fetch(ix + 1, iy - 1 + j, z) + cx[3] * (int) fetch(ix + 2, iy - 1 + j, z);
					r[j] = UpTraits<T>::is_signed ? signed_fixed_round(s) : unsigned_fixed_round(s);
				}
				const int s = cy[0] * r[0] + cy[1] * r[1] + cy[2] * r[2] + cy[3] * r[3];
				int v = UpTraits<T>::is_signed ? signed_fixed_round(s) : unsigned_fixed_round(s);
				v = min(max(v, UpTraits<T>::ilo), UpTraits<T>::ihi);
				q[z] = (T) v;
			}
		}
		else {
			const double *cx = tables->mf[tx];
			const double *cy = tables->mf[ty];
			double nx[4], ny[4];
			if (std::is_same<T, double>::value) {
				// double images: no table, the coefficients of the exact offsets (bicubic_notab)
				catmull_device(nx, __dsub_rn(x, (double) ix));
				catmull_device(ny, __dsub_rn(y, (double) iy));
				cx = nx;
				cy = ny;
			}
			for (int z = 0; z < bands; z++) {
				double r[4];
#pragma unroll
				for (int j = 0; j < 4; j++) {
					r[j] = dot4(cx[0], (double) fetch(ix - 1, iy - 1 + j, z), cx[1], (double) fetch(ix, iy - 1 + j, z), cx[2],
						(double) fetch(ix + 1, iy - 1 + j, z), cx[3], (double) fetch(ix + 2, iy - 1 + j, z));
					if (std::is_same<T, float>::value)
						r[j] = (double) (float) r[j]; // cubic_float<float> returns a float
				}
				double v = dot4(cy[0], r[0], cy[1], r[1], cy[2], r[2], cy[3], r[3]);
				if (!std::is_floating_point<T>::value) {
					// VIPS_CLIP(lo, v, hi), then the C conversion
					v = v < UpTraits<T>::lo() ? UpTraits<T>::lo() : (v > UpTraits<T>::hi() ? UpTraits<T>::hi() : v);
				}
				q[z] = vh::cvt_to<T>(v);
			}
		}
	}
}

} // namespace vh
