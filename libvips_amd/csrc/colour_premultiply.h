// Part of colour.hip, which includes it: vips_premultiply and vips_unpremultiply for gfx950 (conversion/premultiply.c,
// unpremultiply.c), ONE kernel per region -- the kernels, their launcher and the C ABI.
#pragma once

#include "colour_device.h"
#include "colour_rows.h"

#include <type_traits>

namespace vh {

struct PremulArgs {
	const unsigned char *in;
	unsigned char *out;
	long long in_stride, out_stride;
	int width, height, bands;
	double max_alpha;
	int scale[256]; // the uchar fast path's table (premultiply.c:252-258, unpremultiply.c:316-323)
};

// fast uchar -> uchar path: premultiply.c:163-176, unpremultiply.c:222-235
__global__ void __launch_bounds__(256)
premul_u8_kernel(PremulArgs a)
{
	__shared__ int scale[256];
	scale[threadIdx.x] = a.scale[threadIdx.x];
	__syncthreads();
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= a.width)
		return;
	if (a.bands == 4) {
		for (int y0 = blockIdx.y * RU; y0 < a.height; y0 += gridDim.y * RU) {
			unsigned int vv[RU];
#pragma unroll
			for (int r = 0; r < RU; r++) {
				const int y = min(y0 + r, a.height - 1);
				vv[r] = *reinterpret_cast<const unsigned int *>(a.in + (long long) y * a.in_stride + (long long) x * 4);
			}
#pragma unroll
			for (int r = 0; r < RU; r++) {
				if (y0 + r >= a.height)
					break;
				const unsigned int v = vv[r];
				const unsigned int alpha = v >> 24;
				const int s = scale[alpha];
				const unsigned int cr = ((int) (v & 0xff) * s + 128) >> 8;
				const unsigned int cg = ((int) ((v >> 8) & 0xff) * s + 128) >> 8;
				const unsigned int cb = ((int) ((v >> 16) & 0xff) * s + 128) >> 8;
				*reinterpret_cast<unsigned int *>(a.out + (long long) (y0 + r) * a.out_stride + (long long) x * 4) =
					(cr & 0xff) | ((cg & 0xff) << 8) | ((cb & 0xff) << 16) | (alpha << 24);
			}
		}
		return;
	}
	for (int y = blockIdx.y; y < a.height; y += gridDim.y) {
		const unsigned char *p = a.in + (long long) y * a.in_stride + (long long) x * a.bands;
		unsigned char *q = a.out + (long long) y * a.out_stride + (long long) x * a.bands;
		{
			const int alpha = p[a.bands - 1];
			const int s = scale[alpha];
			for (int i = 0; i < a.bands - 1; i++)
				q[i] = (unsigned char) ((p[i] * s + 128) >> 8);
			q[a.bands - 1] = (unsigned char) alpha;
		}
	}
}

// PRE_MANY / PRE_RGBA (premultiply.c:78-128) and UNPRE / FUNPRE (unpremultiply.c:85-186),
// float output.
// one pixel of NB bands (alpha last); ptr-free so that the vector path stays in registers
template <typename TIN, bool INVERSE, int NB>
static __device__ __forceinline__ void premul_pixel(const TIN (&p)[NB], float (&q)[NB], double max_alpha)
{
	constexpr int ab = NB - 1;
	const TIN alpha = p[ab];
	// VIPS_CLIP(0, alpha, max_alpha) is evaluated in double
	double clip = (double) alpha;
	clip = max_alpha < clip ? max_alpha : clip;
	clip = 0.0 > clip ? 0.0 : clip;
	if (!INVERSE) {
		// IN clip_alpha = CLIP(...); OUT nalpha = (OUT) clip_alpha / max_alpha
		const TIN clip_alpha = vh::cvt_to<TIN>(clip);
		const float nalpha = (float) __ddiv_rn((double) (float) clip_alpha, max_alpha);
#pragma unroll
		for (int i = 0; i < ab; i++)
			q[i] = __fmul_rn((float) p[i], nalpha);
		q[ab] = (float) alpha;
	}
	else {
		float factor;
		if (sizeof(TIN) == 4 && ((TIN) 0.5f != (TIN) 0)) // float input: FUNPRE
			factor = fabs((double) alpha) < 0.01 ? 0.0f : (float) __ddiv_rn(max_alpha, (double) alpha);
		else
			factor = alpha == (TIN) 0 ? 0.0f : (float) __ddiv_rn(max_alpha, (double) alpha);
#pragma unroll
		for (int i = 0; i < ab; i++)
			q[i] = __fmul_rn(factor, (float) p[i]);
		q[ab] = (float) clip;
	}
}

// RGBA with aligned rows: one vector load and one 16-byte store per pixel (a wave writes 1 KiB of a line per
// instruction), RU rows in flight per lane.  8-bit alpha: what premul_pixel makes of an alpha value -- the factor
// (a double division) and the alpha it writes -- is a 256-entry table the block fills with premul_pixel itself
// (1.0f * factor == factor), so a pixel is three multiplies.  Round 5's form (a row per turn, the division per
// pixel) ran at 62 % of 8 TB/s.
template <typename TIN, bool INVERSE>
__global__ void __launch_bounds__(256)
premul_rgba_kernel(PremulArgs a)
{
	constexpr bool TABLE = sizeof(TIN) == 1;
	__shared__ float2 s_tab[TABLE ? 256 : 1];
	if constexpr (TABLE) {
		const TIN one[4] = { (TIN) 1, (TIN) 1, (TIN) 1, (TIN) (unsigned char) threadIdx.x };
		float q[4];
		premul_pixel<TIN, INVERSE, 4>(one, q, a.max_alpha);
		s_tab[threadIdx.x] = make_float2(q[0], q[3]);
		__syncthreads();
	}
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= a.width)
		return;
	for (int y0 = blockIdx.y * RU; y0 < a.height; y0 += gridDim.y * RU) {
		Vec4<TIN> pv[RU];
#pragma unroll
		for (int r = 0; r < RU; r++)
			pv[r] = ((const Vec4<TIN> *) (a.in + (long long) min(y0 + r, a.height - 1) * a.in_stride))[x];
#pragma unroll
		for (int r = 0; r < RU; r++) {
			if (y0 + r >= a.height)
				break;
			float qv[4];
			if constexpr (TABLE) {
				const float2 e = s_tab[(unsigned char) pv[r].v[3]];
#pragma unroll
				for (int i = 0; i < 3; i++)
					qv[i] = INVERSE ? __fmul_rn(e.x, (float) pv[r].v[i]) : __fmul_rn((float) pv[r].v[i], e.x);
				qv[3] = e.y;
			}
			else
				premul_pixel<TIN, INVERSE, 4>(pv[r].v, qv, a.max_alpha);
			((float4 *) (a.out + (long long) (y0 + r) * a.out_stride))[x] = make_float4(qv[0], qv[1], qv[2], qv[3]);
		}
	}
}

template <typename TIN, bool INVERSE>
__global__ void __launch_bounds__(256)
premul_float_kernel(PremulArgs a)
{
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= a.width)
		return;
	const int ab = a.bands - 1;
	for (int y = blockIdx.y; y < a.height; y += gridDim.y) {
		const TIN *p = (const TIN *) (a.in + (long long) y * a.in_stride) + (long long) x * a.bands;
		float *q = (float *) (a.out + (long long) y * a.out_stride) + (long long) x * a.bands;
		const TIN alpha = p[ab];
		// VIPS_CLIP(0, alpha, max_alpha) is evaluated in double
		double clip = (double) alpha;
		clip = a.max_alpha < clip ? a.max_alpha : clip;
		clip = 0.0 > clip ? 0.0 : clip;
		if (!INVERSE) {
			// IN clip_alpha = CLIP(...); OUT nalpha = (OUT) clip_alpha / max_alpha
			const TIN clip_alpha = vh::cvt_to<TIN>(clip);
			const float nalpha = (float) __ddiv_rn((double) (float) clip_alpha, a.max_alpha);
			for (int i = 0; i < ab; i++)
				q[i] = __fmul_rn((float) p[i], nalpha);
			q[ab] = (float) alpha;
		}
		else {
			float factor;
			if (sizeof(TIN) == 4 && ((TIN) 0.5f != (TIN) 0)) // float input: FUNPRE
				factor = fabs((double) alpha) < 0.01 ? 0.0f : (float) __ddiv_rn(a.max_alpha, (double) alpha);
			else
				factor = alpha == (TIN) 0 ? 0.0f : (float) __ddiv_rn(a.max_alpha, (double) alpha);
			for (int i = 0; i < ab; i++)
				q[i] = __fmul_rn(factor, (float) p[i]);
			q[ab] = (float) clip;
		}
	}
}

int premultiply_region(const VipsHipRegion *in, const VipsHipRegion *out, double max_alpha, int uchar,
	int inverse)
{
	const char *domain = inverse ? "unpremultiply" : "premultiply";
	if (ensure_init())
		return -1;
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (in->bands != out->bands || in->bands < 2) {
		error(domain, "need the same number of bands (at least 2) in and out");
		return -1;
	}
	if (out->left < in->left || out->top < in->top ||
		out->left + out->width > in->left + in->width ||
		out->top + out->height > in->top + in->height) {
		error(domain, "input region too small");
		return -1;
	}
	const bool fast = uchar && in->format == VIPS_HIP_FORMAT_UCHAR;
	if (out->format != (fast ? VIPS_HIP_FORMAT_UCHAR : VIPS_HIP_FORMAT_FLOAT)) {
		error(domain, "output region has the wrong format");
		return -1;
	}
	PremulArgs a;
	const int ies = format_sizeof(in->format);
	a.in = (const unsigned char *) in->data + (size_t) (out->top - in->top) * in->stride +
		(size_t) (out->left - in->left) * in->bands * ies;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) out->stride;
	a.width = out->width;
	a.height = out->height;
	a.bands = in->bands;
	a.max_alpha = max_alpha;
	for (int i = 0; i < 256; i++) {
		double clip = (double) i;
		clip = max_alpha < clip ? max_alpha : clip;
		clip = 0.0 > clip ? 0.0 : clip;
		if (inverse)
			a.scale[i] = clip == 0 ? 0 : (int) (256 * max_alpha / clip);
		else
			a.scale[i] = (int) (256 * clip / max_alpha);
	}
	dim3 block(256, 1, 1);
	dim3 grid((a.width + 255) / 256, rows_grid((a.width + 255) / 256, a.height), 1);
	Gate gate(inverse ? "unpremultiply" : "premultiply");
	if (fast) {
		if (a.bands == 4 && (((uintptr_t) a.in | (uintptr_t) a.out | a.in_stride | a.out_stride) & 3)) {
			error(domain, "RGBA rows must be 4-byte aligned");
			return -1;
		}
		hipLaunchKernelGGL(premul_u8_kernel, grid, block, 0, stream(), a);
	}
	else {
#define GO(TIN) \
	if (a.bands == 4 && !(((uintptr_t) a.in | (uintptr_t) a.in_stride) % (4 * sizeof(TIN))) && \
		!(((uintptr_t) a.out | (uintptr_t) a.out_stride) & 15) && !getenv("VIPS_HIP_NO_PREMUL_RGBA")) { \
		if (inverse) \
			hipLaunchKernelGGL((premul_rgba_kernel<TIN, true>), grid, block, 0, stream(), a); \
		else \
			hipLaunchKernelGGL((premul_rgba_kernel<TIN, false>), grid, block, 0, stream(), a); \
	} \
	else if (inverse) \
		hipLaunchKernelGGL((premul_float_kernel<TIN, true>), grid, block, 0, stream(), a); \
	else \
		hipLaunchKernelGGL((premul_float_kernel<TIN, false>), grid, block, 0, stream(), a); \
	break;
		switch (in->format) {
		case VIPS_HIP_FORMAT_UCHAR: GO(unsigned char)
		case VIPS_HIP_FORMAT_CHAR: GO(signed char)
		case VIPS_HIP_FORMAT_USHORT: GO(unsigned short)
		case VIPS_HIP_FORMAT_SHORT: GO(short)
		case VIPS_HIP_FORMAT_UINT: GO(unsigned int)
		case VIPS_HIP_FORMAT_INT: GO(int)
		case VIPS_HIP_FORMAT_FLOAT: GO(float)
		default:
			error(domain, "band format %d is outside the HIP path", in->format);
			return -1;
		}
#undef GO
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

} // namespace vh

using namespace vh;

extern "C" {

int vips_hip_premultiply_gen(const VipsHipRegion *in, const VipsHipRegion *out, double max_alpha,
	int uchar, int inverse)
{
	return premultiply_region(in, out, max_alpha, uchar, inverse);
}

} // extern "C"
