// Colour path for gfx950: the per-scanline process_line functions of colour/
// (colour.c:119-156 drives them one scanline at a time) as ONE kernel per region.
//
// A colourspace conversion in the reference is a chain of images, each step
// rounding its result to float (or uchar / short) in memory:
//     sRGB -> LAB = cast(uchar), sRGB2scRGB, scRGB2XYZ, XYZ2Lab   (colourspace.c:362)
// Every step is per-pixel, so the chain is evaluated here in registers with the same
// intermediate types and the same operation order: one read and one write per pixel
// instead of four of each, identical bits.  Transcendentals never run on the device:
// the LUTs the reference builds with powf()/cbrtf() (LabQ2sRGB.c:130-160,
// XYZ2Lab.c:92-106) are built on the host by the same libm calls and uploaded.
//
// Float arithmetic: the reference is compiled for baseline x86-64 (SSE2, no FMA), so
// every multiply and add below is a separate IEEE operation (__fmul_rn/__fadd_rn,
// __dmul_rn/...; the file is also built with -ffp-contract=off).
#include "colour_device.h"
#include "colour_rows.h"
#define VH_CBRT_FN static __host__ __device__ __forceinline__
#include "cbrt_exact.h"
#include "cbrt_quad.h"

#include <climits>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <map>
#include <mutex>
#include <type_traits>

namespace vh {

// One thread per pixel.  TIN/TOUT are the in-memory band formats.
template <typename TIN, typename TOUT>
__global__ void __launch_bounds__(256)
colour_route_kernel(RouteArgs a)
{
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= a.width)
		return;
	for (int y0 = blockIdx.y * RU; y0 < a.height; y0 += gridDim.y * RU) {
		TIN i0[RU], i1[RU], i2[RU];
#pragma unroll
		for (int r = 0; r < RU; r++) {
			const int y = min(y0 + r, a.height - 1);
			const TIN *p = (const TIN *) (a.in + (long long) y * a.in_stride) + (long long) x * a.in_bands;
			i0[r] = p[0];
			i1[r] = p[1];
			i2[r] = p[2];
		}
#pragma unroll
		for (int r = 0; r < RU; r++) {
			const int y = y0 + r;
			if (y < a.height) {
				const TIN *p = (const TIN *) (a.in + (long long) y * a.in_stride) + (long long) x * a.in_bands;
				TOUT *q = (TOUT *) (a.out + (long long) y * a.out_stride) + (long long) x * a.out_bands;
				route_pixel<TIN, TOUT>(a, a.tables.v2Y_8, a.tables.Y2v_8, i0[r], i1[r], i2[r], q[0], q[1], q[2]);
				for (int e = 0; e < a.extra_bands; e++)
					q[3 + e] = Carry<TIN, TOUT>::run(p[3 + e], a.alpha_scale);
			}
		}
	}
}

// 3 bands -> 3 bands, 4 pixels per thread: the 12 input elements arrive as three aligned
// vector loads and the 12 outputs leave as three aligned vector stores (dword / dwordx2 /
// dwordx4 for 1 / 2 / 4-byte elements).  One element per store instruction, as the scalar
// kernel does for interleaved bands, makes every wave store touch all of the wave's cache
// lines (3x the L1->L2 write requests); this is the shape of every BASELINE colour config
// (C3: float -> float, thumbnails: uchar -> float / short and back).
template <typename TIN, typename TOUT, int ROUTE>
__global__ void __launch_bounds__(256)
colour_route_x4_kernel(RouteArgs a)
{
	// the two 8-bit tables in LDS: up to six of a pixel's table reads stay off the vector memory path
	__shared__ float s_v2Y[256];
	__shared__ int s_Y2v[260];
	s_v2Y[threadIdx.x] = a.tables.v2Y_8[threadIdx.x];
	s_Y2v[threadIdx.x] = a.tables.Y2v_8[threadIdx.x];
	if (threadIdx.x == 0)
		s_Y2v[256] = a.tables.Y2v_8[256];
	__syncthreads();
	const int x4 = blockIdx.x * blockDim.x + threadIdx.x;
	if (x4 * 4 >= a.width)
		return;
	for (int y = blockIdx.y; y < a.height; y += gridDim.y) {
		const Vec4<TIN> *p = (const Vec4<TIN> *) (a.in + (long long) y * a.in_stride) + (long long) x4 * 3;
		Vec4<TOUT> *q = (Vec4<TOUT> *) (a.out + (long long) y * a.out_stride) + (long long) x4 * 3;
		const Vec4<TIN> v0 = p[0], v1 = p[1], v2 = p[2];
		Vec4<TOUT> r0, r1, r2;
		route_pixel<TIN, TOUT, ROUTE>(a, s_v2Y, s_Y2v, v0.v[0], v0.v[1], v0.v[2], r0.v[0], r0.v[1], r0.v[2]);
		route_pixel<TIN, TOUT, ROUTE>(a, s_v2Y, s_Y2v, v0.v[3], v1.v[0], v1.v[1], r0.v[3], r1.v[0], r1.v[1]);
		route_pixel<TIN, TOUT, ROUTE>(a, s_v2Y, s_Y2v, v1.v[2], v1.v[3], v2.v[0], r1.v[2], r1.v[3], r2.v[0]);
		route_pixel<TIN, TOUT, ROUTE>(a, s_v2Y, s_Y2v, v2.v[1], v2.v[2], v2.v[3], r2.v[1], r2.v[2], r2.v[3]);
		q[0] = r0;
		q[1] = r1;
		q[2] = r2;
	}
}

// Routes whose pel changes shape: 1 colour band in (BW2sRGB / GREY162RGB16 first: the band stands for R, G and B),
// 1 colour band out (scRGB2BW* last), or the shift casts of the sRGB / RGB16 pair (no colour step at all:
// a.n_steps == 0, every band through shift_cast).  One thread per pixel, any band count, extra bands carried as
// colour_route_kernel does: the stepwise path of images with alpha, the region form, odd widths.
template <typename TIN, typename TOUT>
__global__ void __launch_bounds__(256)
colour_mono_kernel(RouteArgs a)
{
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= a.width)
		return;
	for (int y0 = blockIdx.y * RU; y0 < a.height; y0 += gridDim.y * RU) {
		TIN i0[RU], i1[RU], i2[RU];
#pragma unroll
		for (int r = 0; r < RU; r++) {
			const int y = min(y0 + r, a.height - 1);
			const TIN *p = (const TIN *) (a.in + (long long) y * a.in_stride) + (long long) x * a.in_bands;
			i0[r] = p[0];
			i1[r] = i2[r] = i0[r];
			if (a.in_colour == 3) {
				i1[r] = p[1];
				i2[r] = p[2];
			}
		}
#pragma unroll
		for (int r = 0; r < RU; r++) {
			const int y = y0 + r;
			if (y < a.height) {
				const TIN *p = (const TIN *) (a.in + (long long) y * a.in_stride) + (long long) x * a.in_bands;
				TOUT *q = (TOUT *) (a.out + (long long) y * a.out_stride) + (long long) x * a.out_bands;
				TOUT o0, o1, o2;
				if (a.n_steps)
					route_pixel<TIN, TOUT>(a, a.tables.v2Y_8, a.tables.Y2v_8, i0[r], i1[r], i2[r], o0, o1, o2);
				else {
					o0 = shift_cast<TOUT, TIN>(i0[r]);
					o1 = shift_cast<TOUT, TIN>(i1[r]);
					o2 = shift_cast<TOUT, TIN>(i2[r]);
				}
				q[0] = o0;
				if (a.out_colour == 3) {
					q[1] = o1;
					q[2] = o2;
				}
				for (int e = 0; e < a.extra_bands; e++)
					q[a.out_colour + e] = a.n_steps ? Carry<TIN, TOUT>::run(p[a.in_colour + e], a.alpha_scale)
													: shift_cast<TOUT, TIN>(p[a.in_colour + e]);
			}
		}
	}
}

// 3 bands -> grey, 4 pixels per thread: decode, luminance, encode in registers; the 12 input elements arrive as
// three aligned vector loads and the 4 grey values leave as ONE store of 4 (uchar) or 8 (ushort) bytes -- a byte
// store per lane would make every wave store a partial write of one cache line.  The 8-bit tables in LDS as in
// colour_route_x4_kernel.  DEC: the routes of the colour spaces an image is usually in, compiled in -- 1 the 8-bit
// sRGB decode (sRGB2scRGB, scRGB2BW*), 2 the 16-bit one (sRGB2scRGB16, scRGB2BW*), 3 none (scRGB2BW* alone); the
// depth of the encode is TOUT's.  0: the steps are read at run time (any route that ends in scRGB2BW*).
template <typename TIN, typename TOUT, int DEC>
static __device__ __forceinline__ TOUT grey_pixel(const RouteArgs &a, const float *v2Y8, const int *Y2v8, TIN i0, TIN i1, TIN i2)
{
	if constexpr (DEC == 0) {
		TOUT g, u1, u2;
		route_pixel<TIN, TOUT>(a, v2Y8, Y2v8, i0, i1, i2, g, u1, u2);
		return g;
	}
	else {
		float R, G, B;
		if constexpr (DEC == 1) {
			R = v2Y8[load_as_uchar_like<TIN>(i0, 255)];
			G = v2Y8[load_as_uchar_like<TIN>(i1, 255)];
			B = v2Y8[load_as_uchar_like<TIN>(i2, 255)];
		}
		else if constexpr (DEC == 2) {
			R = a.tables.v2Y_16[load_as_uchar_like<TIN>(i0, 65535)];
			G = a.tables.v2Y_16[load_as_uchar_like<TIN>(i1, 65535)];
			B = a.tables.v2Y_16[load_as_uchar_like<TIN>(i2, 65535)];
		}
		else {
			R = (float) i0;
			G = (float) i1;
			B = (float) i2;
		}
		if constexpr (sizeof(TOUT) == 2)
			return (TOUT) scRGB2BW_value(a.tables.Y2v_16, R, G, B, 65535);
		else
			return (TOUT) scRGB2BW_value(Y2v8, R, G, B, 255);
	}
}

template <typename TIN, typename TOUT, int DEC>
__global__ void __launch_bounds__(256)
colour_grey_x4_kernel(RouteArgs a)
{
	__shared__ float s_v2Y[256];
	__shared__ int s_Y2v[260];
	s_v2Y[threadIdx.x] = a.tables.v2Y_8[threadIdx.x];
	s_Y2v[threadIdx.x] = a.tables.Y2v_8[threadIdx.x];
	if (threadIdx.x == 0)
		s_Y2v[256] = a.tables.Y2v_8[256];
	__syncthreads();
	const int x4 = blockIdx.x * blockDim.x + threadIdx.x;
	if (x4 * 4 >= a.width)
		return;
	for (int y = blockIdx.y; y < a.height; y += gridDim.y) {
		const Vec4<TIN> *p = (const Vec4<TIN> *) (a.in + (long long) y * a.in_stride) + (long long) x4 * 3;
		Vec4<TOUT> *q = (Vec4<TOUT> *) (a.out + (long long) y * a.out_stride) + x4;
		const Vec4<TIN> v0 = p[0], v1 = p[1], v2 = p[2];
		Vec4<TOUT> g;
		g.v[0] = grey_pixel<TIN, TOUT, DEC>(a, s_v2Y, s_Y2v, v0.v[0], v0.v[1], v0.v[2]);
		g.v[1] = grey_pixel<TIN, TOUT, DEC>(a, s_v2Y, s_Y2v, v0.v[3], v1.v[0], v1.v[1]);
		g.v[2] = grey_pixel<TIN, TOUT, DEC>(a, s_v2Y, s_Y2v, v1.v[2], v1.v[3], v2.v[0]);
		g.v[3] = grey_pixel<TIN, TOUT, DEC>(a, s_v2Y, s_Y2v, v2.v[1], v2.v[2], v2.v[3]);
		*q = g;
	}
}

// Grey to grey is a function of one value: B_W -> GREY16 of a uchar (256 ushort entries) and GREY16 -> B_W of a
// ushort (65536 uchar entries, 64 KB: it fits the 160 KB of LDS of a CU twice).  The table is made on the device by
// the route's own steps (grey_table_kernel: route_pixel over every input value, so the table IS the route), kept per
// device, and applied by one streaming kernel: persistent blocks copy it into LDS once, then every lane takes 16
// pixels per trip with 16-byte loads and stores.
template <typename TIN, typename TOUT>
__global__ void __launch_bounds__(256)
grey_table_kernel(RouteArgs a, TOUT *table, int n)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	TOUT o0, o1, o2;
	route_pixel<TIN, TOUT>(a, a.tables.v2Y_8, a.tables.Y2v_8, (TIN) i, (TIN) i, (TIN) i, o0, o1, o2);
	table[i] = o0;
}

struct GreyLutArgs {
	const unsigned char *in;
	unsigned char *out;
	long long in_stride, out_stride;
	int width, height; // (a contiguous image is handed over as one long row)
	int vec;           // rows start and advance on 16-byte boundaries on both sides
	const void *table;
};

template <typename T, int N>
struct alignas(16) Pack {
	T v[N];
};

template <typename TIN, typename TOUT>
__global__ void __launch_bounds__(sizeof(TIN) == 2 ? 1024 : 256)
grey_lut_kernel(GreyLutArgs a)
{
	constexpr int N = sizeof(TIN) == 2 ? 65536 : 256;
	__shared__ __attribute__((aligned(16))) TOUT s_tab[N];
	for (int i = threadIdx.x; i < N * (int) sizeof(TOUT) / 16; i += blockDim.x)
		((Pack<unsigned int, 4> *) s_tab)[i] = ((const Pack<unsigned int, 4> *) a.table)[i];
	__syncthreads();
	const int per_row = (a.width + 15) / 16;
	const long long chunks = (long long) per_row * a.height;
	for (long long c = (long long) blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (long long) gridDim.x * blockDim.x) {
		const int y = (int) (c / per_row);
		const int x = (int) (c - (long long) y * per_row) * 16;
		const TIN *p = (const TIN *) (a.in + (long long) y * a.in_stride) + x;
		TOUT *q = (TOUT *) (a.out + (long long) y * a.out_stride) + x;
		if (a.vec && x + 16 <= a.width) {
			const Pack<TIN, 16> v = *(const Pack<TIN, 16> *) p;
			Pack<TOUT, 16> r;
#pragma unroll
			for (int k = 0; k < 16; k++)
				r.v[k] = s_tab[v.v[k]];
			*(Pack<TOUT, 16> *) q = r;
		}
		else {
			const int n = min(16, a.width - x);
			for (int k = 0; k < n; k++)
				q[k] = s_tab[p[k]];
		}
	}
}

// sRGB -> Lab / LabS of 3-band uchar or float images with XYZ2Lab's cube-root table in LDS
// (cbrt_exact.h: every entry bit for bit from 34 KB): a lane that gathers from the 400 KB table in
// global memory pulls a 128-byte line through its CU's L1 fill path per channel (~146 cycles of that
// path per wave instruction, tools/gather_probe.hip), which bounded colour_route_x4_kernel on these
// routes; here a pixel reads nothing but its own bytes.  Persistent blocks (the tables are copied
// once per block), 4 pixels per thread, rows dealt round the grid.
// F32: the table's single-precision form (cbrt_exact.h), when the host found that its cbrtf fits it
template <typename TIN, bool LABS, bool F32>
__global__ void __launch_bounds__(256)
colour_lab_lds_kernel(RouteArgs a, CbrtExact cx)
{
	__shared__ float s_v2Y[256];
	__shared__ unsigned int s_res[CBRT_RES_WORDS];
	__shared__ CbrtBlockD s_bd[F32 ? 1 : CBRT_BLOCKS + 1];
	__shared__ CbrtBlockF s_bf[F32 ? CBRT_BLOCKS + 1 : 1];
	__shared__ CbrtBlockI s_bi[CBRT_BLOCKS + 1];
	__shared__ float s_lin[CBRT_LINEAR];
	const int t = threadIdx.x;
	s_v2Y[t] = a.tables.v2Y_8[t];
	for (int i = t; i < CBRT_RES_WORDS; i += 256)
		s_res[i] = F32 ? cx.res32[i] : cx.res[i];
	for (int i = t; i < CBRT_LINEAR; i += 256)
		s_lin[i] = cx.lin[i];
	if (t <= CBRT_BLOCKS) {
		if constexpr (F32)
			s_bf[t] = cx.bf[t];
		else
			s_bd[t] = cx.bd[t];
		s_bi[t] = cx.bi[t];
	}
	__syncthreads();
	const CbrtExact lds = { s_bd, s_bi, s_res, s_lin, s_bf, s_res };
	const int x4 = blockIdx.x * blockDim.x + t;
	if (x4 * 4 >= a.width)
		return;
	typedef typename std::conditional<LABS, short, float>::type TOUT;
	for (int y = blockIdx.y; y < a.height; y += gridDim.y) {
		const Vec4<TIN> *p = (const Vec4<TIN> *) (a.in + (long long) y * a.in_stride) + (long long) x4 * 3;
		Vec4<TOUT> *q = (Vec4<TOUT> *) (a.out + (long long) y * a.out_stride) + (long long) x4 * 3;
		const Vec4<TIN> v0 = p[0], v1 = p[1], v2 = p[2];
		const TIN in[12] = { v0.v[0], v0.v[1], v0.v[2], v0.v[3], v1.v[0], v1.v[1], v1.v[2], v1.v[3], v2.v[0], v2.v[1], v2.v[2],
			v2.v[3] };
		TOUT out[12];
#pragma unroll
		for (int m = 0; m < 4; m++) {
			// sRGB2scRGB.c:72-90 (vips_colour_code_build casts to uchar), scRGB2XYZ.c:58-82
			Px v;
			v.a = s_v2Y[load_as_uchar_like<TIN>(in[3 * m], 255)];
			v.b = s_v2Y[load_as_uchar_like<TIN>(in[3 * m + 1], 255)];
			v.c = s_v2Y[load_as_uchar_like<TIN>(in[3 * m + 2], 255)];
			v = step_scRGB2XYZ(v);
			// XYZ2Lab.c:109-138 on small finite values
			const float n0 = quant_div_finite<0>(__fmul_rn(100000.0f, v.a));
			const float n1 = quant_div_finite<1>(__fmul_rn(100000.0f, v.b));
			const float n2 = quant_div_finite<2>(__fmul_rn(100000.0f, v.c));
			const int i0 = min(max(vh::cvt_i32(n0), 0), CBRT_N - 2);
			const int i1 = min(max(vh::cvt_i32(n1), 0), CBRT_N - 2);
			const int i2 = min(max(vh::cvt_i32(n2), 0), CBRT_N - 2);
			float t0, dt;
			if constexpr (F32)
				cbrt_pair32(lds, i0, &t0, &dt);
			else
				cbrt_pair(lds, i0, &t0, &dt);
			const float cbx = __fadd_rn(t0, __fmul_rn(__fsub_rn(n0, (float) i0), dt));
			if constexpr (F32)
				cbrt_pair32(lds, i1, &t0, &dt);
			else
				cbrt_pair(lds, i1, &t0, &dt);
			const float cby = __fadd_rn(t0, __fmul_rn(__fsub_rn(n1, (float) i1), dt));
			if constexpr (F32)
				cbrt_pair32(lds, i2, &t0, &dt);
			else
				cbrt_pair(lds, i2, &t0, &dt);
			const float cbz = __fadd_rn(t0, __fmul_rn(__fsub_rn(n2, (float) i2), dt));
			const float L = __fsub_rn(__fmul_rn(116.0F, cby), 16.0F);
			const float A = __fmul_rn(500.0F, __fsub_rn(cbx, cby));
			const float B = __fmul_rn(200.0F, __fsub_rn(cby, cbz));
			if constexpr (LABS) {
				out[3 * m] = lab2labs_finite(L, 32767.0 / 100.0, 0.0);
				out[3 * m + 1] = lab2labs_finite(A, 32768.0 / 128.0, -32768.0);
				out[3 * m + 2] = lab2labs_finite(B, 32768.0 / 128.0, -32768.0);
			}
			else {
				out[3 * m] = L;
				out[3 * m + 1] = A;
				out[3 * m + 2] = B;
			}
		}
		Vec4<TOUT> r0 = { { out[0], out[1], out[2], out[3] } }, r1 = { { out[4], out[5], out[6], out[7] } },
				   r2 = { { out[8], out[9], out[10], out[11] } };
		q[0] = r0;
		q[1] = r1;
		q[2] = r2;
	}
}

// ... with the table in cbrt_quad.h's form: 27 vector instructions and two LDS reads per channel instead of ~45
// and seven (one 16-byte block record, the pair's residual bits), 57 KB of LDS: two blocks per CU
// (1024 threads: ONE block's tables serve a CU's 16 waves -- 256-thread blocks, two per CU by their LDS, left two
// waves per SIMD to hide the LDS reads behind and ran no faster than the older form)
template <typename TIN, bool LABS>
__global__ void __launch_bounds__(1024)
colour_lab_quad_kernel(RouteArgs a, CbrtQuad cq)
{
	__shared__ float s_v2Y[256];
	__shared__ unsigned int s_res[CBQ_RES_WORDS];
	__shared__ __attribute__((aligned(16))) CbqBlock s_blk[CBQ_BLOCKS];
	const int t = threadIdx.x;
	if (t < 256)
		s_v2Y[t] = a.tables.v2Y_8[t];
	for (int i = t; i < CBQ_RES_WORDS; i += 1024)
		s_res[i] = cq.res[i];
	for (int i = t; i < CBQ_BLOCKS; i += 1024)
		s_blk[i] = cq.blk[i];
	__syncthreads();
	const int x4 = blockIdx.x * blockDim.x + t;
	if (x4 * 4 >= a.width)
		return;
	typedef typename std::conditional<LABS, short, float>::type TOUT;
	// (the next row's pixels travel while this row's are converted: with 600 instructions between a load and its
	// store a wave otherwise sits out the whole memory latency once per 4 pixels)
	Vec4<TIN> n0, n1, n2;
	{
		const Vec4<TIN> *p = (const Vec4<TIN> *) (a.in + (long long) blockIdx.y * a.in_stride) + (long long) x4 * 3;
		n0 = p[0];
		n1 = p[1];
		n2 = p[2];
	}
	for (int y = blockIdx.y; y < a.height; y += gridDim.y) {
		Vec4<TOUT> *q = (Vec4<TOUT> *) (a.out + (long long) y * a.out_stride) + (long long) x4 * 3;
		const Vec4<TIN> v0 = n0, v1 = n1, v2 = n2;
		if (y + (int) gridDim.y < a.height) {
			const Vec4<TIN> *p = (const Vec4<TIN> *) (a.in + (long long) (y + (int) gridDim.y) * a.in_stride) + (long long) x4 * 3;
			n0 = p[0];
			n1 = p[1];
			n2 = p[2];
		}
		const TIN in[12] = { v0.v[0], v0.v[1], v0.v[2], v0.v[3], v1.v[0], v1.v[1], v1.v[2], v1.v[3], v2.v[0], v2.v[1], v2.v[2],
			v2.v[3] };
		TOUT out[12];
#pragma unroll
		for (int m = 0; m < 4; m++) {
			// sRGB2scRGB.c:72-90 (vips_colour_code_build casts to uchar), scRGB2XYZ.c:58-82
			Px v;
			v.a = s_v2Y[load_as_uchar_like<TIN>(in[3 * m], 255)];
			v.b = s_v2Y[load_as_uchar_like<TIN>(in[3 * m + 1], 255)];
			v.c = s_v2Y[load_as_uchar_like<TIN>(in[3 * m + 2], 255)];
			v = step_scRGB2XYZ(v);
			// XYZ2Lab.c:109-138 on small finite values
			const float n[3] = { quant_div_finite<0>(__fmul_rn(100000.0f, v.a)), quant_div_finite<1>(__fmul_rn(100000.0f, v.b)),
				quant_div_finite<2>(__fmul_rn(100000.0f, v.c)) };
			float cb[3];
#pragma unroll
			for (int c = 0; c < 3; c++) {
				const int i = min(max(vh::cvt_i32(n[c]), 0), CBRT_N - 2);
				const float fi = (float) i;
				float t0, dt;
				cbq_pair(s_blk, s_res, i, fi, &t0, &dt);
				cb[c] = __fadd_rn(t0, __fmul_rn(__fsub_rn(n[c], fi), dt));
			}
			const float L = __fsub_rn(__fmul_rn(116.0F, cb[1]), 16.0F);
			const float A = __fmul_rn(500.0F, __fsub_rn(cb[0], cb[1]));
			const float B = __fmul_rn(200.0F, __fsub_rn(cb[1], cb[2]));
			if constexpr (LABS) {
				out[3 * m] = lab2labs_finite(L, 32767.0 / 100.0, 0.0);
				out[3 * m + 1] = lab2labs_finite(A, 32768.0 / 128.0, -32768.0);
				out[3 * m + 2] = lab2labs_finite(B, 32768.0 / 128.0, -32768.0);
			}
			else {
				out[3 * m] = L;
				out[3 * m + 1] = A;
				out[3 * m + 2] = B;
			}
		}
		Vec4<TOUT> r0 = { { out[0], out[1], out[2], out[3] } }, r1 = { { out[4], out[5], out[6], out[7] } },
				   r2 = { { out[8], out[9], out[10], out[11] } };
		q[0] = r0;
		q[1] = r1;
		q[2] = r2;
	}
}

// ----------------------------------------------------------- route launcher

int colour_route_prepare(const int *steps, int n_steps, RouteArgs *a)
{
	ColourTables tables;
	if (n_steps < 1 || n_steps > 8 || ensure_init() || colour_tables(&tables))
		return -1;
	memset(a, 0, sizeof(*a));
	a->n_steps = n_steps;
	for (int s = 0; s < 8; s++)
		a->steps[s] = s < n_steps ? steps[s] : -1;
	a->alpha_scale = 1.0;
	a->in_bands = a->out_bands = 3;
	a->tables = tables;
	return 0;
}

static inline bool is_replicate(int step)
{
	return step == VIPS_HIP_COLOUR_BW2sRGB || step == VIPS_HIP_COLOUR_GREY162RGB16;
}

static inline bool is_shift(int step)
{
	return step == VIPS_HIP_COLOUR_sRGB2RGB16 || step == VIPS_HIP_COLOUR_RGB162sRGB;
}

// the launches of a route with a band-replicating first step, a grey last step or a shift cast (checked by
// colour_route): the kernel sees the 3-band steps in between (none: the pel goes through shift_cast, a copy when
// the format stays)
static int colour_route_mono(const int *steps, int n_steps, double alpha_scale, const VipsHipRegion *in,
	const VipsHipRegion *out, int in_colour, int out_colour)
{
	const char *domain = "colour";
	RouteArgs a;
	memset(&a, 0, sizeof(a));
	const int ies = format_sizeof(in->format), oes = format_sizeof(out->format);
	a.in = (const unsigned char *) in->data + (size_t) (out->top - in->top) * in->stride +
		(size_t) (out->left - in->left) * in->bands * ies;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) out->stride;
	a.width = out->width;
	a.height = out->height;
	a.in_bands = in->bands;
	a.out_bands = out->bands;
	a.in_colour = in_colour;
	a.out_colour = out_colour;
	a.extra_bands = in->bands - in_colour;
	a.alpha_scale = alpha_scale;
	if (colour_tables(&a.tables))
		return -1;
	a.n_steps = 0;
	for (int s = 0; s < n_steps; s++)
		if (!is_replicate(steps[s]) && !is_shift(steps[s]))
			a.steps[a.n_steps++] = steps[s];
	for (int s = a.n_steps; s < 8; s++)
		a.steps[s] = -1;

	const dim3 block(256, 1, 1);
	// 3 bands to 1, rows that start and advance on 4-element boundaries: 4 pixels per thread, one store of 4 greys
	if (in_colour == 3 && out_colour == 1 && in->bands == 3 && a.n_steps && !(a.width & 3) &&
		!((uintptr_t) a.in % (4 * ies)) && !((uintptr_t) a.out % (4 * oes)) && !(a.in_stride % (4 * ies)) &&
		!(a.out_stride % (4 * oes))) {
		const dim3 grid4((a.width / 4 + 255) / 256, a.height < 32768 ? a.height : 32768, 1);
		Gate gate("colour_grey_x4");
		// (the compiled-in routes, for the formats they are met with)
		int dec = 0;
		if (a.n_steps == 2 && a.steps[0] == VIPS_HIP_COLOUR_sRGB2scRGB &&
			(in->format == VIPS_HIP_FORMAT_UCHAR || in->format == VIPS_HIP_FORMAT_USHORT))
			dec = 1;
		else if (a.n_steps == 2 && a.steps[0] == VIPS_HIP_COLOUR_sRGB2scRGB16 && in->format == VIPS_HIP_FORMAT_USHORT)
			dec = 2;
		else if (a.n_steps == 1 && in->format == VIPS_HIP_FORMAT_FLOAT)
			dec = 3;
#define GREY(TIN, FIN, DEC) \
	if (in->format == FIN && dec == DEC) { \
		if (oes == 1) \
			hipLaunchKernelGGL((colour_grey_x4_kernel<TIN, unsigned char, DEC>), grid4, block, 0, stream(), a); \
		else \
			hipLaunchKernelGGL((colour_grey_x4_kernel<TIN, unsigned short, DEC>), grid4, block, 0, stream(), a); \
		VH_CHECK(hipGetLastError()); \
		return 0; \
	}
		GREY(unsigned char, VIPS_HIP_FORMAT_UCHAR, 1)
		GREY(unsigned short, VIPS_HIP_FORMAT_USHORT, 1)
		GREY(unsigned short, VIPS_HIP_FORMAT_USHORT, 2)
		GREY(float, VIPS_HIP_FORMAT_FLOAT, 3)
		GREY(unsigned char, VIPS_HIP_FORMAT_UCHAR, 0)
		GREY(unsigned short, VIPS_HIP_FORMAT_USHORT, 0)
		GREY(short, VIPS_HIP_FORMAT_SHORT, 0)
		GREY(float, VIPS_HIP_FORMAT_FLOAT, 0)
#undef GREY
	}
	const dim3 grid((a.width + 255) / 256, rows_grid((a.width + 255) / 256, a.height), 1);
	Gate gate("colour_mono");
#define GO(TIN, TOUT) hipLaunchKernelGGL((colour_mono_kernel<TIN, TOUT>), grid, block, 0, stream(), a)
#define GO_IN(TOUT) \
	switch (in->format) { \
	case VIPS_HIP_FORMAT_UCHAR: GO(unsigned char, TOUT); break; \
	case VIPS_HIP_FORMAT_USHORT: GO(unsigned short, TOUT); break; \
	case VIPS_HIP_FORMAT_SHORT: GO(short, TOUT); break; \
	case VIPS_HIP_FORMAT_FLOAT: GO(float, TOUT); break; \
	default: \
		error(domain, "input band format %d is outside the HIP colour path", in->format); \
		return -1; \
	}
	switch (out->format) {
	case VIPS_HIP_FORMAT_UCHAR: GO_IN(unsigned char) break;
	case VIPS_HIP_FORMAT_USHORT: GO_IN(unsigned short) break;
	case VIPS_HIP_FORMAT_SHORT: GO_IN(short) break;
	default: GO_IN(float) break;
	}
#undef GO_IN
#undef GO
	VH_CHECK(hipGetLastError());
	return 0;
}

// B_W -> GREY16 (to16) or GREY16 -> B_W of a one-band image through the route's table: 0 done, -1 error
int grey_lut_image(const VipsHipRegion *in, const VipsHipRegion *out, bool to16)
{
	const char *domain = "colour";
	ColourTables colour;
	if (ensure_init() || check_region(domain, in) || check_region(domain, out) || colour_tables(&colour))
		return -1;
	const int fin = to16 ? VIPS_HIP_FORMAT_UCHAR : VIPS_HIP_FORMAT_USHORT;
	const int fout = to16 ? VIPS_HIP_FORMAT_USHORT : VIPS_HIP_FORMAT_UCHAR;
	if (in->bands != 1 || out->bands != 1 || in->format != fin || out->format != fout || in->width != out->width ||
		in->height != out->height || in->left != out->left || in->top != out->top) {
		error(domain, "the grey table takes a one-band image in its space's own format");
		return -1;
	}
	// the table of this device: the route's steps over every value the input format holds
	static std::mutex &mutex = *new std::mutex;
	static void *tables[64][2];
	const int dev = current_device() < 0 ? 0 : current_device() & 63;
	void *table;
	{
		std::lock_guard<std::mutex> lock(mutex);
		if (!tables[dev][to16]) {
			const int n = to16 ? 256 : 65536;
			const std::vector<unsigned char> zero((size_t) n * (to16 ? 2 : 1), 0);
			void *t = upload(zero.data(), zero.size());
			if (!t)
				return -1;
			RouteArgs a;
			memset(&a, 0, sizeof(a));
			a.tables = colour;
			a.in_colour = a.out_colour = 3;
			a.alpha_scale = 1.0;
			a.n_steps = 2;
			for (int s = 2; s < 8; s++)
				a.steps[s] = -1;
			a.steps[0] = to16 ? VIPS_HIP_COLOUR_sRGB2scRGB : VIPS_HIP_COLOUR_sRGB2scRGB16;
			a.steps[1] = to16 ? VIPS_HIP_COLOUR_scRGB2BW16 : VIPS_HIP_COLOUR_scRGB2BW;
			if (to16)
				hipLaunchKernelGGL((grey_table_kernel<unsigned char, unsigned short>), dim3(1), dim3(256), 0, stream(), a,
					(unsigned short *) t, n);
			else
				hipLaunchKernelGGL((grey_table_kernel<unsigned short, unsigned char>), dim3(256), dim3(256), 0, stream(), a,
					(unsigned char *) t, n);
			VH_CHECK(hipGetLastError());
			// (other threads launch on streams of their own: the table is complete before it is published)
			VH_CHECK(hipStreamSynchronize(stream()));
			tables[dev][to16] = t;
		}
		table = tables[dev][to16];
	}
	GreyLutArgs a;
	a.in = (const unsigned char *) in->data;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) out->stride;
	a.width = out->width;
	a.height = out->height;
	a.table = table;
	const int ies = to16 ? 1 : 2, oes = to16 ? 2 : 1;
	if (a.in_stride == (long long) a.width * ies && a.out_stride == (long long) a.width * oes &&
		(long long) a.width * a.height <= INT_MAX) {
		a.width *= a.height;
		a.height = 1;
	}
	a.vec = !((uintptr_t) a.in & 15) && !((uintptr_t) a.out & 15) && (a.height == 1 || (!(a.in_stride & 15) && !(a.out_stride & 15)));
	const int nt = to16 ? 256 : 1024;
	const long long chunks = (long long) ((a.width + 15) / 16) * a.height;
	// persistent blocks: two 64 KB tables fit a CU's LDS, eight blocks of 256 its wave slots
	const long long full = 256 * (to16 ? 8 : 2);
	long long blocks = (chunks + nt - 1) / nt;
	blocks = blocks < 1 ? 1 : blocks > full ? full : blocks;
	Gate gate(to16 ? "grey_lut_u8_u16" : "grey_lut_u16_u8");
	if (to16)
		hipLaunchKernelGGL((grey_lut_kernel<unsigned char, unsigned short>), dim3((unsigned int) blocks), dim3(nt), 0, stream(), a);
	else
		hipLaunchKernelGGL((grey_lut_kernel<unsigned short, unsigned char>), dim3((unsigned int) blocks), dim3(nt), 0, stream(), a);
	VH_CHECK(hipGetLastError());
	return 0;
}

int colour_route(const int *steps, int n_steps, double alpha_scale, const VipsHipRegion *in,
	const VipsHipRegion *out)
{
	const char *domain = "colour";
	if (ensure_init())
		return -1;
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (n_steps < 1 || n_steps > 8) {
		error(domain, "bad route length %d", n_steps);
		return -1;
	}
	// the steps that change the shape of a pel (header: where they may stand); what is left between them is a
	// chain of 3-band steps
	const bool rep = is_replicate(steps[0]);
	const bool shift = is_shift(steps[n_steps - 1]);
	const bool grey_out = steps[n_steps - 1] == VIPS_HIP_COLOUR_scRGB2BW || steps[n_steps - 1] == VIPS_HIP_COLOUR_scRGB2BW16;
	const bool mono = rep || shift || grey_out;
	if (shift && n_steps != (rep ? 2 : 1)) {
		error(domain, "a shift cast stands alone or straight behind a band-replicating step");
		return -1;
	}
	// colour bands of a stored pel (a shift cast on its own treats every band alike: one "colour" band, the rest extra)
	const int in_colour = rep || shift ? 1 : 3;
	const int out_colour = grey_out || (shift && !rep) ? 1 : 3;
	if (in->bands < in_colour) {
		error(domain, "image must have at least %d bands", in_colour); // vips_check_bands_atleast
		return -1;
	}
	if (out->bands - out_colour != in->bands - in_colour) {
		error(domain, mono ? "output must have the input's extra bands behind its colour bands"
						   : "output must have as many bands as the input");
		return -1;
	}
	if (out->left < in->left || out->top < in->top ||
		out->left + out->width > in->left + in->width ||
		out->top + out->height > in->top + in->height) {
		error(domain, "input region too small");
		return -1;
	}
	// what the last step stores
	const int last = steps[n_steps - 1];
	int want_out;
	if (last == VIPS_HIP_COLOUR_scRGB2sRGB || last == VIPS_HIP_COLOUR_scRGB2BW || last == VIPS_HIP_COLOUR_RGB162sRGB)
		want_out = VIPS_HIP_FORMAT_UCHAR;
	else if (last == VIPS_HIP_COLOUR_scRGB2sRGB16 || last == VIPS_HIP_COLOUR_scRGB2BW16 || last == VIPS_HIP_COLOUR_sRGB2RGB16)
		want_out = VIPS_HIP_FORMAT_USHORT;
	else if (last == VIPS_HIP_COLOUR_Lab2LabS)
		want_out = VIPS_HIP_FORMAT_SHORT;
	else if (is_replicate(last))
		want_out = in->format; // (the band three times: the format stays)
	else
		want_out = VIPS_HIP_FORMAT_FLOAT;
	if (out->format != want_out) {
		error(domain, "output region has format %d, this conversion writes %d", out->format, want_out);
		return -1;
	}
	if (shift && in->format != VIPS_HIP_FORMAT_UCHAR && in->format != VIPS_HIP_FORMAT_USHORT) {
		error(domain, "shift casts of band format %d are outside the HIP colour path", in->format);
		return -1;
	}
	for (int s = 0; s < n_steps; s++) {
		const int st = steps[s];
		if (st < 0 || st >= VIPS_HIP_COLOUR_LAST) {
			error(domain, "unknown colour step %d", st);
			return -1;
		}
		const bool decoder = st == VIPS_HIP_COLOUR_sRGB2scRGB || st == VIPS_HIP_COLOUR_sRGB2scRGB16 ||
			st == VIPS_HIP_COLOUR_LabS2Lab;
		const bool encoder = st == VIPS_HIP_COLOUR_scRGB2sRGB || st == VIPS_HIP_COLOUR_scRGB2sRGB16 ||
			st == VIPS_HIP_COLOUR_Lab2LabS || st == VIPS_HIP_COLOUR_scRGB2BW || st == VIPS_HIP_COLOUR_scRGB2BW16 ||
			is_shift(st);
		if ((decoder && s != (rep ? 1 : 0)) || (encoder && s != n_steps - 1) || (is_replicate(st) && s != 0)) {
			error(domain, "colour step %d cannot sit at position %d of a fused route", st, s);
			return -1;
		}
	}
	ColourTables tables;
	if (colour_tables(&tables))
		return -1;
	if (mono)
		return colour_route_mono(steps, n_steps, alpha_scale, in, out, in_colour, out_colour);

	RouteArgs a;
	const int ies = format_sizeof(in->format);
	a.in = (const unsigned char *) in->data + (size_t) (out->top - in->top) * in->stride +
		(size_t) (out->left - in->left) * in->bands * ies;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) out->stride;
	a.width = out->width;
	a.height = out->height;
	a.in_bands = in->bands;
	a.out_bands = out->bands;
	a.n_steps = n_steps;
	for (int s = 0; s < 8; s++)
		a.steps[s] = s < n_steps ? steps[s] : -1;
	a.extra_bands = in->bands - 3;
	a.alpha_scale = alpha_scale;
	a.tables = tables;

	dim3 block(256, 1, 1);
	dim3 grid((a.width + 255) / 256, rows_grid((a.width + 255) / 256, a.height), 1);
	// (a gate name per kernel family, given where the launch is chosen: a report says which one ran)
	// 3 bands in and out, rows that start and advance on 4-element boundaries: 4 pixels per thread
	const int oes = format_sizeof(want_out);
	const bool x4 = in->bands == 3 && out->bands == 3 && !(a.width & 3) &&
		!((uintptr_t) a.in % (4 * ies)) && !((uintptr_t) a.out % (4 * oes)) &&
		!(a.in_stride % (4 * ies)) && !(a.out_stride % (4 * oes));
	// (one row per block: the table-gathering route kernels measured faster with many short blocks)
	const dim3 grid4((a.width / 4 + 255) / 256, a.height < 32768 ? a.height : 32768, 1);
	// the routes with their steps compiled in (colour_device.h kStaticRoutes), for the formats they
	// are met with: sRGB -> Lab / LabS from uchar and float, LabS / Lab -> sRGB uchar
	int route_id = 0;
	for (int r = 1; r < kStaticRouteCount && x4; r++)
		if (n_steps == kStaticRoutes[r][0] && !memcmp(steps, &kStaticRoutes[r][1], sizeof(int) * n_steps))
			route_id = r;
	bool launched = false;
	// sRGB -> Lab / LabS from uchar or float: the cube-root table from LDS (colour_lab_lds_kernel)
	if ((route_id == 1 || route_id == 2) && !getenv("VIPS_HIP_NO_LAB_LDS") &&
		(in->format == VIPS_HIP_FORMAT_UCHAR || in->format == VIPS_HIP_FORMAT_FLOAT)) {
		const CbrtQuad *cq = cbrt_quad_tables();
		const CbrtExact *cx = cq ? nullptr : cbrt_exact_tables();
		if (cq) {
			Gate gate("colour_lab_quad");
			const int gx = (a.width / 4 + 1023) / 1024;
			int gy = (256 + gx - 1) / gx; // one block of 1024 per CU, each walking its share of the rows
			const char *e = getenv("VIPS_HIP_LAB_QUAD_GRID");
			if (e && atoi(e) > 0)
				gy = (atoi(e) + gx - 1) / gx;
			gy = gy > a.height ? a.height : gy;
			const dim3 gridp(gx, gy, 1), blockq(1024, 1, 1);
			if (route_id == 1 && in->format == VIPS_HIP_FORMAT_UCHAR)
				hipLaunchKernelGGL((colour_lab_quad_kernel<unsigned char, false>), gridp, blockq, 0, stream(), a, *cq);
			else if (route_id == 1)
				hipLaunchKernelGGL((colour_lab_quad_kernel<float, false>), gridp, blockq, 0, stream(), a, *cq);
			else if (in->format == VIPS_HIP_FORMAT_UCHAR)
				hipLaunchKernelGGL((colour_lab_quad_kernel<unsigned char, true>), gridp, blockq, 0, stream(), a, *cq);
			else
				hipLaunchKernelGGL((colour_lab_quad_kernel<float, true>), gridp, blockq, 0, stream(), a, *cq);
			launched = true;
		}
		else if (cx) {
			Gate gate("colour_lab_lds");
			const int gx = (a.width / 4 + 255) / 256;
			int gy = (256 * 4 + gx - 1) / gx; // four 34 KB blocks per CU, each walking its share of the rows
			gy = gy > a.height ? a.height : gy;
			const dim3 gridp(gx, gy, 1);
			const bool f32 = cx->bf != nullptr;
#define LAB_LDS(TIN, LABS) \
	do { \
		if (f32) \
			hipLaunchKernelGGL((colour_lab_lds_kernel<TIN, LABS, true>), gridp, block, 0, stream(), a, *cx); \
		else \
			hipLaunchKernelGGL((colour_lab_lds_kernel<TIN, LABS, false>), gridp, block, 0, stream(), a, *cx); \
	} while (0)
			if (route_id == 1 && in->format == VIPS_HIP_FORMAT_UCHAR)
				LAB_LDS(unsigned char, false);
			else if (route_id == 1)
				LAB_LDS(float, false);
			else if (in->format == VIPS_HIP_FORMAT_UCHAR)
				LAB_LDS(unsigned char, true);
			else
				LAB_LDS(float, true);
#undef LAB_LDS
			launched = true;
		}
		else
			vips_hip_error_clear();
	}
#define STATIC_ROUTE(R, TIN, FIN, TOUT, FOUT) \
	if (!launched && route_id == R && in->format == FIN && want_out == FOUT) { \
		Gate gate("colour_route_x4_static"); \
		hipLaunchKernelGGL((colour_route_x4_kernel<TIN, TOUT, R>), grid4, block, 0, stream(), a); \
		launched = true; \
	}
	STATIC_ROUTE(1, float, VIPS_HIP_FORMAT_FLOAT, float, VIPS_HIP_FORMAT_FLOAT)
	STATIC_ROUTE(1, unsigned char, VIPS_HIP_FORMAT_UCHAR, float, VIPS_HIP_FORMAT_FLOAT)
	STATIC_ROUTE(2, float, VIPS_HIP_FORMAT_FLOAT, short, VIPS_HIP_FORMAT_SHORT)
	STATIC_ROUTE(2, unsigned char, VIPS_HIP_FORMAT_UCHAR, short, VIPS_HIP_FORMAT_SHORT)
	STATIC_ROUTE(3, short, VIPS_HIP_FORMAT_SHORT, unsigned char, VIPS_HIP_FORMAT_UCHAR)
	STATIC_ROUTE(4, float, VIPS_HIP_FORMAT_FLOAT, unsigned char, VIPS_HIP_FORMAT_UCHAR)
#undef STATIC_ROUTE
#define GO(TIN, TOUT) \
	if (launched) \
		; \
	else if (x4) { \
		Gate gate("colour_route_x4"); \
		hipLaunchKernelGGL((colour_route_x4_kernel<TIN, TOUT, 0>), grid4, block, 0, stream(), a); \
	} \
	else { \
		Gate gate("colour_route"); \
		hipLaunchKernelGGL((colour_route_kernel<TIN, TOUT>), grid, block, 0, stream(), a); \
	}
#define GO_IN(TOUT) \
	switch (in->format) { \
	case VIPS_HIP_FORMAT_UCHAR: GO(unsigned char, TOUT); break; \
	case VIPS_HIP_FORMAT_USHORT: GO(unsigned short, TOUT); break; \
	case VIPS_HIP_FORMAT_SHORT: GO(short, TOUT); break; \
	case VIPS_HIP_FORMAT_FLOAT: GO(float, TOUT); break; \
	default: \
		error(domain, "input band format %d is outside the HIP colour path", in->format); \
		return -1; \
	}
	switch (want_out) {
	case VIPS_HIP_FORMAT_UCHAR: GO_IN(unsigned char) break;
	case VIPS_HIP_FORMAT_USHORT: GO_IN(unsigned short) break;
	case VIPS_HIP_FORMAT_SHORT: GO_IN(short) break;
	default: GO_IN(float) break;
	}
#undef GO_IN
#undef GO
	VH_CHECK(hipGetLastError());
	return 0;
}

} // namespace vh

using namespace vh;

extern "C" {

int vips_hip_colour_gen(int step, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return colour_route(&step, 1, 1.0, in, out);
}

int vips_hip_colour_route_gen(const int *steps, int n_steps, double alpha_scale,
	const VipsHipRegion *in, const VipsHipRegion *out)
{
	return colour_route(steps, n_steps, alpha_scale, in, out);
}

} // extern "C"

// The other pointwise families of this translation unit, a file each.  (One unit: tests/emul replaces a kernel object
// by the twin of its .hip, and every kernel template keeps one instantiation.)
#include "colour_cast.h"
#include "colour_sharpen.h"
#include "colour_premultiply.h"
