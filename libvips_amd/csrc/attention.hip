// The two kernels vips_smartcrop's attention search (conversion/smartcrop.c:204-320) needs beside the operations
// the library has: the point-wise chain between the colour conversions and the blur, and vips_max.  Both work on
// the image the search shrinks its input to (about 32 x 32 pels), so neither is written for speed: what matters is
// that every value is the float the reference's chain of float images holds at that step -- each operation below
// is one IEEE operation, rounded where the reference stores an image (no contraction: the __f*_rn forms).
//
//   attention_score   per pel, from the XYZ image, its 3 x 3 edge convolution and its Lab image:
//                       edge  = | 5 * conv(Y) |                                   (linear1 5 0, abs: float)
//                       n     = XYZ / sqrt(X^2 + Y^2 + Z^2), 0 where that is 0     (pythagoras, divide)
//                       skin  = -100 * | n - (0.78, 0.57, 0.44) | + 100            (linear in double, pythagoras, linear1)
//                       out   = (edge + (Y > 5 ? skin : 0)) + (Y > 5 ? a : 0)      (more_const, ifthenelse, sum)
//                     vips_pow_const1(x, 0.5) is sqrt of the double, 0 for 0 (arithmetic/math2.c:147-162).
//   attention_max     ONE block: the largest value, and of the pels that hold it the first in raster order -- the
//                     pel vips_max reports, which takes a later pel only when it is strictly greater
//                     (arithmetic/max.c:334-349); NaNs never count.  Writes { value, x, y } (x = -1: no pel counts).
#include "gcn.h"
#include "internal.h"
#include "kernel_stmt.h"

#include <cmath>
#include <cstdint>

namespace vh {

constexpr int ATT_THREADS = 256;

struct AttentionArgs {
	const unsigned char *xyz, *edge, *lab; // 3-band float images
	unsigned char *out;                    // 1-band float
	long long xyz_stride, edge_stride, lab_stride, out_stride;
	int width, height;
};

// sqrt(b0^2 + b1^2 + b2^2) as smartcrop.c's pythagoras() makes it: float squares, vips_sum's float sum in band
// order, the square root of the double stored as float
VH_DEV float att_pythagoras(float b0, float b1, float b2)
{
	const float sum = __fadd_rn(__fadd_rn(__fmul_rn(b0, b0), __fmul_rn(b1, b1)), __fmul_rn(b2, b2));
	return sum == 0.0f ? 0.0f : (float) sqrt((double) sum);
}

__global__ void __launch_bounds__(ATT_THREADS)
attention_score_kernel(AttentionArgs a)
{
	const int n = a.width * a.height;
	for (int i = (int) (blockIdx.x * ATT_THREADS + threadIdx.x); i < n; i += (int) gridDim.x * ATT_THREADS) {
		const int y = i / a.width, x = i - y * a.width;
		const float *xyz = (const float *) (a.xyz + (long long) y * a.xyz_stride) + 3 * x;
		const float *edge = (const float *) (a.edge + (long long) y * a.edge_stride) + 3 * x;
		const float *lab = (const float *) (a.lab + (long long) y * a.lab_stride) + 3 * x;
		const float X = xyz[0], Y = xyz[1], Z = xyz[2];

		const float e = fabsf(__fadd_rn(__fmul_rn(5.0f, edge[1]), 0.0f));

		const float mag = att_pythagoras(X, Y, Z);
		const float n0 = mag == 0.0f ? 0.0f : __fdiv_rn(X, mag);
		const float n1 = mag == 0.0f ? 0.0f : __fdiv_rn(Y, mag);
		const float n2 = mag == 0.0f ? 0.0f : __fdiv_rn(Z, mag);
		// vips_linear with vector constants works in double: 1.0 * n + c, stored as float
		const float d0 = (float) __dadd_rn(__dmul_rn(1.0, (double) n0), -0.78);
		const float d1 = (float) __dadd_rn(__dmul_rn(1.0, (double) n1), -0.57);
		const float d2 = (float) __dadd_rn(__dmul_rn(1.0, (double) n2), -0.44);
		const float dist = att_pythagoras(d0, d1, d2);
		const float skin = __fadd_rn(__fmul_rn(-100.0f, dist), 100.0f);

		const bool lit = Y > 5.0f;
		const float s = lit ? skin : 0.0f;
		const float sat = lit ? lab[1] : 0.0f;
		float *out = (float *) (a.out + (long long) y * a.out_stride) + x;
		*out = __fadd_rn(__fadd_rn(e, s), sat);
	}
}

struct AttentionMaxArgs {
	const unsigned char *in; // 1-band float
	long long stride;
	int width, height;
	unsigned int *result; // { the value's bits, x, y }
};

__global__ void __launch_bounds__(ATT_THREADS)
attention_max_kernel(AttentionMaxArgs a)
{
	__shared__ float best_v[ATT_THREADS];
	__shared__ int best_i[ATT_THREADS];
	const int tid = (int) threadIdx.x;
	const int n = a.width * a.height;
	float v = 0.0f;
	int at = -1;
	for (int i = tid; i < n; i += ATT_THREADS) {
		const int y = i / a.width, x = i - y * a.width;
		const float p = ((const float *) (a.in + (long long) y * a.stride))[x];
		if (p != p)
			continue;
		if (at < 0 || p > v) { // (a thread meets its pels in raster order: an equal value later on is not taken)
			v = p;
			at = i;
		}
	}
	best_v[tid] = v;
	best_i[tid] = at;
	__syncthreads();
	if (tid == 0) {
		for (int t = 1; t < ATT_THREADS; t++) {
			const int ti = best_i[t];
			if (ti < 0)
				continue;
			const float tv = best_v[t];
			if (at < 0 || tv > v || (tv == v && ti < at)) {
				v = tv;
				at = ti;
			}
		}
		a.result[0] = __builtin_bit_cast(unsigned int, v);
		a.result[1] = at < 0 ? 0xffffffffu : (unsigned int) (at % a.width);
		a.result[2] = at < 0 ? 0xffffffffu : (unsigned int) (at / a.width);
	}
}

static int att_check(const char *domain, const _VipsHipImage *im, int bands, int width, int height)
{
	if (!im || im->format != VIPS_HIP_FORMAT_FLOAT || im->bands != bands || im->width != width || im->height != height) {
		error(domain, "attention: a step of the search gave an image of another shape");
		return -1;
	}
	return 0;
}

int attention_score(const char *domain, const _VipsHipImage *xyz, const _VipsHipImage *edge, const _VipsHipImage *lab,
	_VipsHipImage *out)
{
	if (!xyz || att_check(domain, xyz, 3, xyz->width, xyz->height) || att_check(domain, edge, 3, xyz->width, xyz->height) ||
		att_check(domain, lab, 3, xyz->width, xyz->height) || att_check(domain, out, 1, xyz->width, xyz->height))
		return -1;
	if ((long long) xyz->width * xyz->height >= (1LL << 30)) {
		error(domain, "attention: image too large");
		return -1;
	}
	AttentionArgs a = {};
	a.xyz = (const unsigned char *) xyz->data;
	a.edge = (const unsigned char *) edge->data;
	a.lab = (const unsigned char *) lab->data;
	a.out = (unsigned char *) out->data;
	a.xyz_stride = (long long) xyz->stride;
	a.edge_stride = (long long) edge->stride;
	a.lab_stride = (long long) lab->stride;
	a.out_stride = (long long) out->stride;
	a.width = xyz->width;
	a.height = xyz->height;
	int blocks = (a.width * a.height + ATT_THREADS - 1) / ATT_THREADS;
	blocks = blocks > 1024 ? 1024 : blocks;
	{
		Gate gate("attention_score");
		hipLaunchKernelGGL(attention_score_kernel, dim3(blocks, 1, 1), dim3(ATT_THREADS, 1, 1), 0, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

int attention_max(const char *domain, const _VipsHipImage *in, unsigned int *result)
{
	if (!in || !result || att_check(domain, in, 1, in->width, in->height))
		return -1;
	if ((long long) in->width * in->height >= (1LL << 30)) {
		error(domain, "attention: image too large");
		return -1;
	}
	AttentionMaxArgs a = {};
	a.in = (const unsigned char *) in->data;
	a.stride = (long long) in->stride;
	a.width = in->width;
	a.height = in->height;
	a.result = result;
	{
		Gate gate("attention_max");
		hipLaunchKernelGGL(attention_max_kernel, dim3(1, 1, 1), dim3(ATT_THREADS, 1, 1), 0, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

} // namespace vh
