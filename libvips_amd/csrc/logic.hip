// vips_relational / vips_relational_const (arithmetic/relational.c), vips_boolean / vips_boolean_const (boolean.c),
// vips_ifthenelse with and without `blend` (conversion/ifthenelse.c) and the band operations vips_bandjoin /
// vips_bandjoin_const / vips_extract_band / vips_bandmean / vips_bandbool (conversion/bandjoin.c, extract.c, bandmean.c,
// bandbool.c) on the device (gfx950).  Every operation is ONE launch that writes every output byte once.
//
//   logic_stream, logic_general   the comparisons and booleans through pointwise.h's two kernels: this file gives them
//                               the expressions (logic_elem) and the policy (LogicOp: the constants of the *_const
//                               operations are staged to LDS); everything under VIPS_HIP_NO_LOGIC_STREAM is general.
//   select_stream<T, BLEND, B>  three operands.  B == 0: the condition has the operands' bands, a lane makes one 16-byte
//                               group and reads the matching 16 / sizeof(T) condition bytes.  B == 2 .. 4: a ONE-band
//                               condition over B-band operands (a mask over RGB): a lane makes B consecutive groups --
//                               16 / sizeof(T) whole pels -- and reads that many condition bytes in one load; which byte
//                               an element takes is known when the kernel is compiled.  B < 0: the same for five bands
//                               and more, the groups in a loop and the byte picked by the element's run-time pel.
//   select_general<T, BLEND>    one element a lane.
//   band_stream<T, OP, B>       the band operations are pel-structured: input and output pels differ in size.  Lanes on
//                               16-byte groups of the OUTPUT row, one global_store_dwordx4.  bandmean and bandbool of
//                               B == 2 .. 4 bands read the B * 16 contiguous bytes that make a group as aligned dwords;
//                               bandjoin (any number of sources from a table in LDS: pointer, stride, elements a pel,
//                               first band, band range of the output; a source without a pointer is a constant),
//                               extract_band and the other band counts gather their elements one load each.
//   band_pels<T, PA, FA, NA, NB, CONSTS>   the common shapes of bandjoin (two images of 1 .. 4 bands), bandjoin_const
//                               (1 .. 4 bands and constants) and extract_band (from pels of 2 .. 4 bands) with every
//                               count a template argument: a lane makes 16 / sizeof(T) whole pels, reads their source
//                               bytes as aligned dwords and stores one dwordx4 for every 16 bytes of them.
//   band_general<T, OP>         one output element a lane: output rows off dwords.
//
// The arithmetic is the reference's, expression by expression (cited in place); the file is compiled with
// -ffp-contract=off, float -> int conversions are v_cvt_i32 by name (vh::cvt_i32).
#include "logic_device.h"
#include "pointwise.h"

namespace vh {

// ---------------------------------------------------------------- the reference's expressions (logic_elem: logic_device.h)

// ifthenelse.c:96-141 for one element: c the condition's uchar
template <typename T>
VH_DEV T blend_elem(u8 c, T a, T b)
{
	if constexpr (std::is_floating_point<T>::value) {
		// FBLEND1 / FBLENDN: const double v = c / 255.0; q = v * a + (1.0 - v) * b, the store rounds
		const f64 v = __ddiv_rn((f64) c, 255.0);
		return (T) (v * (f64) a + (1.0 - v) * (f64) b);
	}
	else if constexpr (std::is_same<T, u32>::value) {
		// IBLEND1 / IBLENDN with an unsigned int pel: the arithmetic is unsigned, modulo 2^32
		const u32 v = c;
		return (v * a + (255u - v) * b + 128u) / 255u;
	}
	else {
		// ... every other pel: int arithmetic, the division truncates toward zero (the sum made modulo 2^32, as the
		// reference's processor makes it)
		const u32 v = c;
		const s32 sum = (s32) (v * (u32) (s32) a + (255u - v) * (u32) (s32) b + 128u);
		return (T) (sum / 255);
	}
}

// bandmean.c:58-106 on a sum; bandbool.c:133-165 on an accumulator
template <typename T>
struct BandSum {
	typedef typename std::conditional<std::is_floating_point<T>::value, T,
		typename std::conditional<sizeof(T) == 4, typename std::conditional<std::is_unsigned<T>::value, u64, long long>::type,
			typename std::conditional<std::is_unsigned<T>::value, u32, s32>::type>::type>::type type;
};

template <typename T>
VH_DEV T band_mean(typename BandSum<T>::type sum, int bands)
{
	typedef typename BandSum<T>::type S;
	if constexpr (std::is_same<T, f32>::value)
		return __fdiv_rn(sum, (f32) bands); // FLOOP: sum / bands
	else if constexpr (std::is_same<T, f64>::value)
		return __ddiv_rn(sum, (f64) bands);
	else if constexpr (std::is_unsigned<T>::value)
		return (T) ((sum + (S) (bands / 2)) / (S) bands); // UILOOP: (sum + bands / 2) / bands
	else
		return (T) (sum > 0 ? (sum + (S) (bands / 2)) / (S) bands : (sum - (S) (bands / 2)) / (S) bands); // SILOOP
}

// the accumulator of bandbool: the pel's type for integers (LOOPB), int for float and double (FLOOPB)
template <typename T>
VH_DEV u32 band_bits(T v)
{
	if constexpr (std::is_floating_point<T>::value)
		return (u32) cvt_i32(v);
	else
		return (u32) v;
}

template <int OP>
VH_DEV u32 band_fold(u32 acc, u32 v)
{
	return OP == BAND_AND ? acc & v : OP == BAND_OR ? acc | v : acc ^ v;
}

// ---------------------------------------------------------------- registers <-> elements

// NB bytes (2, 4, 8 or 16) at an offset that is a multiple of NB (of 4 for 8 and 16), the rest of d zero
template <int NB>
VH_DEV void logic_load_bytes(gptr_in base, unsigned int off, unsigned int (&d)[4])
{
	d[0] = d[1] = d[2] = d[3] = 0;
	if constexpr (NB == 2)
		d[0] = gload16(base, off);
	else if constexpr (NB == 4)
		d[0] = gload32(base, off);
	else if constexpr (NB == 8) {
		unsigned int t[2];
		gload64(base, off, t);
		d[0] = t[0];
		d[1] = t[1];
	}
	else
		gload128(base, off, d);
}

// the constants from the kernel's arguments to LDS: thread i brings element i, picked by selects with constant
// indices (a by-value array indexed at run time would be copied to scratch)
VH_DEV void logic_constants(const LogicArgs &a, int *ci, double *cd)
{
	const int t = tid();
	int vi = 0;
	double vd = 0.0;
#pragma unroll
	for (int i = 0; i < LOGIC_MAX_VECTOR; i++) {
		vi = t == i ? a.c_int[i] : vi;
		vd = t == i ? a.c_double[i] : vd;
	}
	if (t < LOGIC_MAX_VECTOR) {
		ci[t] = vi;
		cd[t] = vd;
	}
	barrier();
}

// ---------------------------------------------------------------- comparisons and booleans: the policy

template <int FAMILY, int OP, bool CONST, typename IN_>
struct LogicOp {
	typedef IN_ IN;
	typedef typename LogicOut<FAMILY, IN>::type OUT;
	typedef LogicArgs Args;
	typedef int CA;
	typedef double CB;
	static constexpr int MAX_VECTOR = LOGIC_MAX_VECTOR;
	static constexpr bool binary = !CONST;
	static constexpr bool constants = CONST;
	VH_DEV void stage(const LogicArgs &a, int *ci, double *cd) { logic_constants(a, ci, cd); }
	VH_DEV OUT elem(const LogicArgs &a, IN l, IN r, int ck, double dk) { return logic_elem<FAMILY, OP, CONST, IN>(l, r, a.is_int != 0, ck, dk); }
};

// ---------------------------------------------------------------- select: one element a lane

template <typename T, bool BLEND>
VH_DEV T select_elem(u8 c, T t, T f)
{
	if constexpr (BLEND)
		return blend_elem<T>(c, t, f);
	else
		return c ? t : f; // ifthenelse.c:441-447
}

template <typename T, bool BLEND>
__global__ void __launch_bounds__(POINTWISE_THREADS)
select_general_kernel(SelectArgs a)
{
	const int e = (int) blockIdx.x * POINTWISE_THREADS + (int) threadIdx.x;
	if (e >= a.elems)
		return;
	const int pel = e / a.bands;
	const int ic = a.bc == 1 ? pel : e, i1 = a.b1 == 1 ? pel : e, i2 = a.b2 == 1 ? pel : e;
	for (int y = (int) blockIdx.y; y < a.height; y += (int) gridDim.y) {
		u8 c = 0;
		T t = (T) 0, f = (T) 0;
		if (pel < a.wc && y < a.hc)
			c = (a.cond + (long long) y * a.cond_stride)[ic];
		if (pel < a.w1 && y < a.h1)
			t = ((const T *) (a.in + (long long) y * a.in_stride))[i1];
		if (pel < a.w2 && y < a.h2)
			f = ((const T *) (a.in2 + (long long) y * a.in2_stride))[i2];
		((T *) (a.out + (long long) y * a.out_stride))[e] = select_elem<T, BLEND>(c, t, f);
	}
}

// ---------------------------------------------------------------- ... B groups of 16 bytes a lane

// byte idx (0 .. 15, a run-time value) of four dwords, by selects: registers cannot be indexed at run time
VH_DEV u8 logic_byte_at(const unsigned int (&c)[4], int idx)
{
	const unsigned int d = idx < 8 ? (idx < 4 ? c[0] : c[1]) : (idx < 12 ? c[2] : c[3]);
	return (u8) (d >> (8 * (idx & 3)));
}

// a.groups counts a lane's units of a row: one group (B == 0), B groups (16 / sizeof(T) pels) otherwise; B < 0: a
// one-band condition over any number of bands -- a.bands groups a unit, the loop over them is not unrolled and the
// element's condition byte is picked by its run-time pel index
template <typename T, bool BLEND, int B>
__global__ void __launch_bounds__(POINTWISE_THREADS)
select_stream_kernel(SelectArgs a)
{
	constexpr int NE = POINTWISE_GROUP / (int) sizeof(T); // elements of a group; pels of a unit where B != 0
	if constexpr (B < 0) {
		const int ng = a.bands;
		const unsigned int total = (unsigned int) a.groups * (unsigned int) a.height;
		for (unsigned int at = (unsigned int) blockIdx.x * POINTWISE_THREADS + (unsigned int) threadIdx.x; at < total; at += (unsigned int) gridDim.x * POINTWISE_THREADS) {
			const int y = (int) (at / (unsigned int) a.groups);
			const int u = (int) (at - (unsigned int) y * (unsigned int) a.groups);
			const int e0 = u * NE * ng;
			const int n = min(NE * ng, a.elems - e0); // < NE * ng: the row's ragged end
			const unsigned long long crow = (unsigned long long) a.cond + (unsigned long long) y * a.cond_stride;
			const unsigned long long irow = (unsigned long long) a.in + (unsigned long long) y * a.in_stride;
			const unsigned long long irow2 = (unsigned long long) a.in2 + (unsigned long long) y * a.in2_stride;
			const unsigned long long orow = (unsigned long long) a.out + (unsigned long long) y * a.out_stride;
			if (n == NE * ng) {
				unsigned int c[4];
				logic_load_bytes<NE>(gptr_in_of(crow), (unsigned int) u * NE, c);
				int pel = 0, k = 0; // of the next element: its pel in the unit, its band in the pel
				for (int j = 0; j < ng; j++) {
					unsigned int d[4], d2[4], w[4] = { 0, 0, 0, 0 };
					const unsigned int off = (unsigned int) e0 * (unsigned int) sizeof(T) + (unsigned int) j * POINTWISE_GROUP;
					gload128(gptr_in_of(irow), off, d);
					gload128(gptr_in_of(irow2), off, d2);
#pragma unroll
					for (int i = 0; i < NE; i++) {
						const u8 cv = logic_byte_at(c, pel);
						group_put<T>(w, i, select_elem<T, BLEND>(cv, group_take<T, 4>(d, i), group_take<T, 4>(d2, i)));
						k++;
						if (k == ng) {
							k = 0;
							pel++;
						}
					}
					gstore128(gptr_out_of(orow) + off, w);
				}
			}
			else {
				for (int i = 0; i < n; i++) {
					const u8 cv = ((const u8 *) crow)[(e0 + i) / ng];
					((T *) orow)[e0 + i] = select_elem<T, BLEND>(cv, ((const T *) irow)[e0 + i], ((const T *) irow2)[e0 + i]);
				}
			}
		}
		return;
	}
	constexpr int NG = B > 0 ? B : 1;
	const unsigned int total = (unsigned int) a.groups * (unsigned int) a.height;
	for (unsigned int at = (unsigned int) blockIdx.x * POINTWISE_THREADS + (unsigned int) threadIdx.x; at < total; at += (unsigned int) gridDim.x * POINTWISE_THREADS) {
		const int y = (int) (at / (unsigned int) a.groups);
		const int u = (int) (at - (unsigned int) y * (unsigned int) a.groups);
		const int e0 = u * NE * NG;
		const int n = min(NE * NG, a.elems - e0); // < NE * NG: the row's ragged end
		const unsigned long long crow = (unsigned long long) a.cond + (unsigned long long) y * a.cond_stride;
		const unsigned long long irow = (unsigned long long) a.in + (unsigned long long) y * a.in_stride;
		const unsigned long long irow2 = (unsigned long long) a.in2 + (unsigned long long) y * a.in2_stride;
		const unsigned long long orow = (unsigned long long) a.out + (unsigned long long) y * a.out_stride;
		if (n == NE * NG) {
			// the condition's NE bytes: those of the group's elements, or of the unit's pels
			unsigned int c[4];
			logic_load_bytes<NE>(gptr_in_of(crow), (unsigned int) u * NE, c);
#pragma unroll
			for (int j = 0; j < NG; j++) {
				unsigned int d[4], d2[4], w[4] = { 0, 0, 0, 0 };
				const unsigned int off = (unsigned int) e0 * (unsigned int) sizeof(T) + (unsigned int) j * POINTWISE_GROUP;
				gload128(gptr_in_of(irow), off, d);
				gload128(gptr_in_of(irow2), off, d2);
#pragma unroll
				for (int i = 0; i < NE; i++) {
					const u8 cv = group_take<u8, 4>(c, B ? (j * NE + i) / NG : i);
					group_put<T>(w, i, select_elem<T, BLEND>(cv, group_take<T, 4>(d, i), group_take<T, 4>(d2, i)));
				}
				gstore128(gptr_out_of(orow) + off, w);
			}
		}
		else {
			for (int i = 0; i < n; i++) {
				const u8 cv = ((const u8 *) crow)[B ? (e0 + i) / NG : e0 + i];
				((T *) orow)[e0 + i] = select_elem<T, BLEND>(cv, ((const T *) irow)[e0 + i], ((const T *) irow2)[e0 + i]);
			}
		}
	}
}

// ---------------------------------------------------------------- the band operations

// the sources from the kernel's arguments to LDS (as logic_constants)
VH_DEV void band_sources(const BandArgs &a, BandSource *src)
{
	const int t = tid();
	BandSource v = a.src[0];
#pragma unroll
	for (int i = 1; i < BAND_MAX_SOURCES; i++)
		if (t == i)
			v = a.src[i];
	if (t < BAND_MAX_SOURCES)
		src[t] = v;
	barrier();
}

// output element (pel, z) of row y of a join: element first + z - begin of the pel of the source whose band range
// holds z, zero outside that source's rectangle (vips__sizealike); a source without a pointer is a constant
template <typename T>
VH_DEV T band_gather(const BandSource *src, int n, int pel, int z, int y)
{
	int i = 0;
	while (i + 1 < n && z >= src[i].end)
		i++;
	const BandSource s = src[i];
	if (!s.in)
		return (T) s.value;
	if (pel >= s.width || y >= s.height)
		return (T) 0;
	return ((const T *) (s.in + (long long) y * s.stride))[(long long) pel * s.pel_elems + s.first + (z - s.begin)];
}

// what a band operation stores: the pel's type, int for bandbool of float and double (bandbool.c:213-216)
template <typename T, int OP>
struct BandOut {
	typedef typename std::conditional<OP == BAND_JOIN || OP == BAND_MEAN, T, typename LogicOut<LOGIC_BOOLEAN, T>::type>::type type;
};

template <typename T, int OP>
VH_DEV typename BandOut<T, OP>::type band_reduce(const T *p, int bands)
{
	typedef typename BandOut<T, OP>::type OUT;
	if constexpr (OP == BAND_MEAN) {
		typename BandSum<T>::type sum = 0;
		for (int j = 0; j < bands; j++)
			sum += p[j];
		return band_mean<T>(sum, bands);
	}
	else {
		u32 acc = band_bits<T>(p[0]);
		for (int j = 1; j < bands; j++)
			acc = band_fold<OP>(acc, band_bits<T>(p[j]));
		return (OUT) acc;
	}
}

template <typename T, int OP>
__global__ void __launch_bounds__(POINTWISE_THREADS)
band_general_kernel(BandArgs a)
{
	typedef typename BandOut<T, OP>::type OUT;
	__shared__ BandSource src[BAND_MAX_SOURCES];
	band_sources(a, src);
	const int e = (int) blockIdx.x * POINTWISE_THREADS + (int) threadIdx.x;
	if (e >= a.elems)
		return;
	const int pel = e / a.out_bands, z = e - pel * a.out_bands;
	for (int y = (int) blockIdx.y; y < a.height; y += (int) gridDim.y) {
		OUT *q = (OUT *) (a.out + (long long) y * a.out_stride);
		if constexpr (OP == BAND_JOIN)
			q[e] = band_gather<T>(src, a.n, pel, z, y);
		else
			q[e] = band_reduce<T, OP>((const T *) (src[0].in + (long long) y * src[0].stride) + (long long) e * src[0].pel_elems, src[0].pel_elems);
	}
}

template <typename T, int OP, int B>
__global__ void __launch_bounds__(POINTWISE_THREADS)
band_stream_kernel(BandArgs a)
{
	typedef typename BandOut<T, OP>::type OUT;
	constexpr int NE = POINTWISE_GROUP / (int) sizeof(OUT);
	__shared__ BandSource src[BAND_MAX_SOURCES];
	band_sources(a, src);
	const unsigned int total = (unsigned int) a.groups * (unsigned int) a.height;
	for (unsigned int at = (unsigned int) blockIdx.x * POINTWISE_THREADS + (unsigned int) threadIdx.x; at < total; at += (unsigned int) gridDim.x * POINTWISE_THREADS) {
		const int y = (int) (at / (unsigned int) a.groups);
		const int g = (int) (at - (unsigned int) y * (unsigned int) a.groups);
		const int e0 = g * NE;
		const int n = min(NE, a.elems - e0); // < NE: the row's ragged end
		const unsigned long long orow = (unsigned long long) a.out + (unsigned long long) y * a.out_stride;
		if constexpr (OP == BAND_JOIN) {
			int pel = e0 / a.out_bands, z = e0 - pel * a.out_bands;
			unsigned int w[4] = { 0, 0, 0, 0 };
#pragma unroll
			for (int i = 0; i < NE; i++) {
				if (i < n) {
					const T v = band_gather<T>(src, a.n, pel, z, y);
					if (n == NE)
						group_put<T>(w, i, v);
					else
						((T *) orow)[e0 + i] = v;
				}
				z++;
				if (z == a.out_bands) {
					z = 0;
					pel++;
				}
			}
			if (n == NE)
				gstore128(gptr_out_of(orow) + (unsigned int) g * POINTWISE_GROUP, w);
		}
		else {
			const unsigned long long irow = (unsigned long long) src[0].in + (unsigned long long) y * src[0].stride;
			if (B > 0 && n == NE) {
				// the group's NE pels are B * NE contiguous elements: B * sizeof(T) / sizeof(OUT) loads of 16 bytes
				// (all the bands of a pel: band_reduce, with the band count known when the kernel is compiled)
				constexpr int NB = B > 0 ? B : 1;
				constexpr int ND = NB * NE * (int) sizeof(T) / 4;
				unsigned int d[ND], w[4] = { 0, 0, 0, 0 };
				group_load<ND>(gptr_in_of(irow), (unsigned int) e0 * (unsigned int) (NB * sizeof(T)), d);
#pragma unroll
				for (int i = 0; i < NE; i++) {
					if constexpr (OP == BAND_MEAN) {
						typename BandSum<T>::type sum = 0;
#pragma unroll
						for (int j = 0; j < NB; j++)
							sum += group_take<T, ND>(d, i * NB + j);
						group_put<OUT>(w, i, band_mean<T>(sum, NB));
					}
					else {
						u32 acc = band_bits<T>(group_take<T, ND>(d, i * NB));
#pragma unroll
						for (int j = 1; j < NB; j++)
							acc = band_fold<OP>(acc, band_bits<T>(group_take<T, ND>(d, i * NB + j)));
						group_put<OUT>(w, i, (OUT) acc);
					}
				}
				gstore128(gptr_out_of(orow) + (unsigned int) g * POINTWISE_GROUP, w);
			}
			else if (n == NE) {
				unsigned int w[4] = { 0, 0, 0, 0 };
#pragma unroll
				for (int i = 0; i < NE; i++)
					group_put<OUT>(w, i, band_reduce<T, OP>((const T *) irow + (long long) (e0 + i) * src[0].pel_elems, src[0].pel_elems));
				gstore128(gptr_out_of(orow) + (unsigned int) g * POINTWISE_GROUP, w);
			}
			else {
				for (int i = 0; i < n; i++)
					((OUT *) orow)[e0 + i] = band_reduce<T, OP>((const T *) irow + (long long) (e0 + i) * src[0].pel_elems, src[0].pel_elems);
			}
		}
	}
}

// ---------------------------------------------------------------- ... whole pels a lane, sources as dwords

// The common shapes of bandjoin, bandjoin_const and extract_band with every count known when the kernel is compiled:
// an output pel is NA elements of source 0 (pels of PA elements, from element FA) followed by NB elements of source 1
// (pels of NB elements) or -- CONSTS -- by NB constants.  A lane makes NE = 16 / sizeof(T) whole pels: it reads the
// PA * 16 (and NB * 16) contiguous bytes of those pels as aligned dwords and stores NA + NB groups of 16 bytes; which
// register an output element comes from is a constant.  A row's ragged last unit goes through band_gather.
template <typename T, int PA, int FA, int NA, int NB, bool CONSTS>
__global__ void __launch_bounds__(POINTWISE_THREADS)
band_pels_kernel(BandArgs a)
{
	constexpr int NE = POINTWISE_GROUP / (int) sizeof(T);
	constexpr int NO = NA + NB;
	constexpr int NB1 = NB > 0 ? NB : 1;
	__shared__ BandSource src[BAND_MAX_SOURCES];
	band_sources(a, src);
	T cv[NB1];
#pragma unroll
	for (int k = 0; k < NB1; k++)
		cv[k] = CONSTS ? (T) src[1 + k].value : (T) 0;
	const int width = a.elems / NO;
	const unsigned long long in0 = (unsigned long long) src[0].in, in1 = (unsigned long long) src[NB > 0 && !CONSTS ? 1 : 0].in;
	const long long stride0 = src[0].stride, stride1 = src[NB > 0 && !CONSTS ? 1 : 0].stride;
	const unsigned int total = (unsigned int) a.groups * (unsigned int) a.height;
	for (unsigned int at = (unsigned int) blockIdx.x * POINTWISE_THREADS + (unsigned int) threadIdx.x; at < total; at += (unsigned int) gridDim.x * POINTWISE_THREADS) {
		const int y = (int) (at / (unsigned int) a.groups);
		const int u = (int) (at - (unsigned int) y * (unsigned int) a.groups);
		const int p0 = u * NE;
		const int n = min(NE, width - p0); // < NE: the row's ragged end
		const unsigned long long orow = (unsigned long long) a.out + (unsigned long long) y * a.out_stride;
		if (n == NE) {
			unsigned int d0[4 * PA], d1[4 * NB1];
			group_load<4 * PA>(gptr_in_of(in0 + (unsigned long long) y * stride0), (unsigned int) u * (unsigned int) (POINTWISE_GROUP * PA), d0);
			if constexpr (NB > 0 && !CONSTS)
				group_load<4 * NB1>(gptr_in_of(in1 + (unsigned long long) y * stride1), (unsigned int) u * (unsigned int) (POINTWISE_GROUP * NB1), d1);
#pragma unroll
			for (int j = 0; j < NO; j++) {
				unsigned int w[4] = { 0, 0, 0, 0 };
#pragma unroll
				for (int i = 0; i < NE; i++) {
					const int flat = j * NE + i, pel = flat / NO, z = flat % NO;
					T v;
					if (z < NA)
						v = group_take<T, 4 * PA>(d0, pel * PA + FA + z);
					else if constexpr (CONSTS)
						v = cv[z - NA < NB1 ? z - NA : 0];
					else
						v = group_take<T, 4 * NB1>(d1, pel * NB1 + (z - NA < NB1 ? z - NA : 0));
					group_put<T>(w, i, v);
				}
				gstore128(gptr_out_of(orow) + ((unsigned int) u * NO + (unsigned int) j) * POINTWISE_GROUP, w);
			}
		}
		else {
			for (int i = 0; i < n * NO; i++)
				((T *) orow)[p0 * NO + i] = band_gather<T>(src, a.n, p0 + i / NO, i % NO, y);
		}
	}
}

// ---------------------------------------------------------------- dispatch

static bool logic_no_stream()
{
	return getenv("VIPS_HIP_NO_LOGIC_STREAM") != nullptr;
}

template <int FAMILY, int OP, bool CONST, typename IN>
static int logic_launch(const char *domain, const LogicArgs &a)
{
	return pointwise_launch<LogicOp<FAMILY, OP, CONST, IN>>(domain, a, "logic_stream", "logic_general", "VIPS_HIP_NO_LOGIC_STREAM");
}

template <int FAMILY, int OP, bool CONST>
static int logic_by_format(const char *domain, int format, const LogicArgs &a)
{
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR: return logic_launch<FAMILY, OP, CONST, u8>(domain, a);
	case VIPS_HIP_FORMAT_CHAR: return logic_launch<FAMILY, OP, CONST, s8>(domain, a);
	case VIPS_HIP_FORMAT_USHORT: return logic_launch<FAMILY, OP, CONST, u16>(domain, a);
	case VIPS_HIP_FORMAT_SHORT: return logic_launch<FAMILY, OP, CONST, s16>(domain, a);
	case VIPS_HIP_FORMAT_UINT: return logic_launch<FAMILY, OP, CONST, u32>(domain, a);
	case VIPS_HIP_FORMAT_INT: return logic_launch<FAMILY, OP, CONST, s32>(domain, a);
	case VIPS_HIP_FORMAT_FLOAT: return logic_launch<FAMILY, OP, CONST, f32>(domain, a);
	case VIPS_HIP_FORMAT_DOUBLE: return logic_launch<FAMILY, OP, CONST, f64>(domain, a);
	default:
		error(domain, "no kernel for format %d", format);
		return -1;
	}
}

template <int FAMILY, bool CONST>
static int logic_by_op(const char *domain, int op, int format, const LogicArgs &a)
{
	switch (op) {
	case 0: return logic_by_format<FAMILY, 0, CONST>(domain, format, a);
	case 1: return logic_by_format<FAMILY, 1, CONST>(domain, format, a);
	case 2: return logic_by_format<FAMILY, 2, CONST>(domain, format, a);
	case 3: return logic_by_format<FAMILY, 3, CONST>(domain, format, a);
	case 4:
		// (more and moreeq of two images reach the kernels as less and lesseq)
		if constexpr (FAMILY == LOGIC_BOOLEAN || CONST)
			return logic_by_format<FAMILY, 4, CONST>(domain, format, a);
		break;
	case 5:
		if constexpr (FAMILY == LOGIC_RELATIONAL && CONST)
			return logic_by_format<FAMILY, 5, CONST>(domain, format, a);
		break;
	default:
		break;
	}
	error(domain, "no kernel for operation %d", op);
	return -1;
}

int logic_run(const char *domain, int family, int op, int format, LogicArgs a)
{
	if (a.elems < 1 || a.height < 1 || a.bands < 1 || a.elems % a.bands) {
		error(domain, "bad image size");
		return -1;
	}
	if ((long long) a.elems * format_sizeof(format) >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	const bool constants = a.in2 == nullptr;
	if (constants && !a.single && a.bands > LOGIC_MAX_VECTOR) {
		error(domain, "vectors of more than %d elements are outside the HIP path", LOGIC_MAX_VECTOR);
		return -1;
	}
	if (family == LOGIC_RELATIONAL) {
		if (constants)
			return logic_by_op<LOGIC_RELATIONAL, true>(domain, op, format, a);
		// relational.c:120-130: more and moreeq of two images are less and lesseq with the operands exchanged
		if (op == RELATIONAL_MORE || op == RELATIONAL_MOREEQ) {
			LogicArgs s = a;
			s.in = a.in2, s.in_stride = a.in2_stride, s.w1 = a.w2, s.h1 = a.h2, s.b1 = a.b2;
			s.in2 = a.in, s.in2_stride = a.in_stride, s.w2 = a.w1, s.h2 = a.h1, s.b2 = a.b1;
			return logic_by_op<LOGIC_RELATIONAL, false>(domain, op == RELATIONAL_MORE ? RELATIONAL_LESS : RELATIONAL_LESSEQ, format, s);
		}
		return logic_by_op<LOGIC_RELATIONAL, false>(domain, op, format, a);
	}
	if (family == LOGIC_BOOLEAN)
		return constants ? logic_by_op<LOGIC_BOOLEAN, true>(domain, op, format, a) : logic_by_op<LOGIC_BOOLEAN, false>(domain, op, format, a);
	error(domain, "no kernel for family %d", family);
	return -1;
}

// ---------------------------------------------------------------- ... select

static bool select_covers(const SelectArgs &a)
{
	const int width = a.elems / a.bands;
	return a.b1 == a.bands && a.b2 == a.bands && a.w1 >= width && a.w2 >= width && a.wc >= width && a.h1 >= a.height &&
		a.h2 >= a.height && a.hc >= a.height && (a.bc == a.bands || a.bc == 1);
}

template <typename T, bool BLEND, int B>
static void select_stream_launch(const SelectArgs &a)
{
	Gate gate("logic_select_stream");
	hipLaunchKernelGGL((select_stream_kernel<T, BLEND, B>), pointwise_stream_grid((long long) a.groups * a.height), dim3(POINTWISE_THREADS, 1, 1), 0,
		stream(), a);
}

template <typename T, bool BLEND>
static int select_launch(const char *domain, SelectArgs a)
{
	if (!on_unit(a.in, a.in_stride, sizeof(T)) || !on_unit(a.in2, a.in2_stride, sizeof(T)) || !on_unit(a.out, a.out_stride, sizeof(T))) {
		error(domain, "rows must start on whole elements");
		return -1;
	}
	constexpr int NE = POINTWISE_GROUP / (int) sizeof(T);
	// a one-band condition over n bands: units of NE pels, n groups (2 .. 4: unrolled); the same bands (one band over
	// one included): of one group
	const int per_unit = a.bc == a.bands ? 1 : a.bands;
	bool streams = !logic_no_stream() && select_covers(a);
	if (streams) {
		SelectArgs j = a;
		const int width = a.elems / a.bands;
		const long long elems = (long long) a.elems * a.height;
		// rows that follow one another without a gap on every side are one long row (as pointwise_join_rows)
		if (a.height == 1)
			j.in_stride = j.in2_stride = j.out_stride = j.cond_stride = 0;
		if (a.height > 1 && a.in_stride == (long long) a.elems * (int) sizeof(T) && a.in2_stride == a.in_stride && a.out_stride == a.in_stride &&
			a.cond_stride == (long long) width * a.bc && a.w1 == width && a.w2 == width && a.wc == width &&
			elems * (long long) sizeof(T) < (1LL << 31)) {
			j.elems = (int) elems;
			j.w1 = j.w2 = j.wc = j.elems / a.bands;
			j.h1 = j.h2 = j.hc = j.height = 1;
			j.in_stride = j.in2_stride = j.out_stride = j.cond_stride = 0;
		}
		const long long units = ((long long) j.elems + NE * per_unit - 1) / (NE * per_unit);
		streams = on_unit(j.in, j.in_stride, 4) && on_unit(j.in2, j.in2_stride, 4) && on_unit(j.out, j.out_stride, 4) &&
			on_unit(j.cond, j.cond_stride, 4) && units * j.height < (1LL << 31);
		if (streams) {
			a = j;
			a.groups = (int) units;
		}
	}
	if (streams) {
		switch (per_unit) {
		case 1: select_stream_launch<T, BLEND, 0>(a); break;
		case 2: select_stream_launch<T, BLEND, 2>(a); break;
		case 3: select_stream_launch<T, BLEND, 3>(a); break;
		case 4: select_stream_launch<T, BLEND, 4>(a); break;
		default: select_stream_launch<T, BLEND, -1>(a); break;
		}
	}
	else {
		const int bx = (a.elems + POINTWISE_THREADS - 1) / POINTWISE_THREADS;
		dim3 grid(bx, pointwise_rows_grid(bx, a.height), 1);
		Gate gate("logic_select_general");
		hipLaunchKernelGGL((select_general_kernel<T, BLEND>), grid, dim3(POINTWISE_THREADS, 1, 1), 0, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

int select_run(const char *domain, int format, int blend, SelectArgs a)
{
	if (a.elems < 1 || a.height < 1 || a.bands < 1 || a.elems % a.bands) {
		error(domain, "bad image size");
		return -1;
	}
	if ((long long) a.elems * format_sizeof(format) >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	if (!blend) {
		// ifthenelse.c:441-447 copies bytes: one kernel a size
		switch (format_sizeof(format)) {
		case 1: return select_launch<u8, false>(domain, a);
		case 2: return select_launch<u16, false>(domain, a);
		case 4: return select_launch<u32, false>(domain, a);
		case 8: return select_launch<u64, false>(domain, a);
		default: break;
		}
	}
	else {
		switch (format) {
		case VIPS_HIP_FORMAT_UCHAR: return select_launch<u8, true>(domain, a);
		case VIPS_HIP_FORMAT_CHAR: return select_launch<s8, true>(domain, a);
		case VIPS_HIP_FORMAT_USHORT: return select_launch<u16, true>(domain, a);
		case VIPS_HIP_FORMAT_SHORT: return select_launch<s16, true>(domain, a);
		case VIPS_HIP_FORMAT_UINT: return select_launch<u32, true>(domain, a);
		case VIPS_HIP_FORMAT_INT: return select_launch<s32, true>(domain, a);
		case VIPS_HIP_FORMAT_FLOAT: return select_launch<f32, true>(domain, a);
		case VIPS_HIP_FORMAT_DOUBLE: return select_launch<f64, true>(domain, a);
		default: break;
		}
	}
	error(domain, "no kernel for format %d", format);
	return -1;
}

// ---------------------------------------------------------------- ... the band operations

template <typename T, int OP, int B>
static void band_stream_launch(const BandArgs &a)
{
	Gate gate("logic_band_stream");
	hipLaunchKernelGGL((band_stream_kernel<T, OP, B>), pointwise_stream_grid((long long) a.groups * a.height), dim3(POINTWISE_THREADS, 1, 1), 0, stream(),
		a);
}

template <typename T, int PA, int FA, int NA, int NB, bool CONSTS>
static void band_pels_launch(const BandArgs &a)
{
	Gate gate("logic_band_pels");
	hipLaunchKernelGGL((band_pels_kernel<T, PA, FA, NA, NB, CONSTS>), pointwise_stream_grid((long long) a.groups * a.height), dim3(POINTWISE_THREADS, 1, 1),
		0, stream(), a);
}

// bandjoin of two images of 1 .. 4 bands each, bandjoin_const of 1 .. 4 bands and 1 .. 4 constants, extract_band from
// pels of 2 .. 4 bands, where every row starts on a dword and every source covers the output: band_pels.  `a` has its
// rows joined already; a.groups becomes the units of a row.
template <typename T>
static bool band_pels_takes(BandArgs &a)
{
	constexpr int NE = POINTWISE_GROUP / (int) sizeof(T);
	const int width = a.elems / a.out_bands;
	const BandSource &s0 = a.src[0];
	int images = 0;
	while (images < a.n && a.src[images].in)
		images++;
	for (int i = images; i < a.n; i++)
		if (a.src[i].in)
			return false;
	if (images < 1 || images > 2 || (images == 2 && a.n != 2) || !on_unit(a.out, a.out_stride, 4))
		return false;
	for (int i = 0; i < images; i++)
		if (!on_unit(a.src[i].in, a.src[i].stride, 4) || a.src[i].width < width || a.src[i].height < a.height)
			return false;
	const int pa = s0.pel_elems, fa = s0.first, na = s0.end - s0.begin, nb = a.out_bands - na;
	const bool consts = images == 1 && nb > 0;
	if (images == 2 && (a.src[1].first != 0 || a.src[1].pel_elems != nb))
		return false;
	if ((long long) (width + NE - 1) / NE * a.height >= (1LL << 31))
		return false;
	const int units = (width + NE - 1) / NE;
#define PELS(PA, FA, NA, NB, C) \
	if (pa == PA && fa == FA && na == NA && nb == NB && consts == C) { \
		a.groups = units; \
		band_pels_launch<T, PA, FA, NA, NB, C>(a); \
		return true; \
	}
#define JOINS(A) \
	PELS(A, 0, A, 1, false) PELS(A, 0, A, 2, false) PELS(A, 0, A, 3, false) PELS(A, 0, A, 4, false) \
	PELS(A, 0, A, 1, true) PELS(A, 0, A, 2, true) PELS(A, 0, A, 3, true) PELS(A, 0, A, 4, true)
	JOINS(1) JOINS(2) JOINS(3) JOINS(4)
	PELS(2, 0, 1, 0, false) PELS(2, 1, 1, 0, false)
	PELS(3, 0, 1, 0, false) PELS(3, 1, 1, 0, false) PELS(3, 2, 1, 0, false) PELS(3, 0, 2, 0, false) PELS(3, 1, 2, 0, false)
	PELS(4, 0, 1, 0, false) PELS(4, 1, 1, 0, false) PELS(4, 2, 1, 0, false) PELS(4, 3, 1, 0, false) PELS(4, 0, 2, 0, false)
	PELS(4, 1, 2, 0, false) PELS(4, 2, 2, 0, false) PELS(4, 0, 3, 0, false) PELS(4, 1, 3, 0, false)
#undef JOINS
#undef PELS
	return false;
}

template <typename T, int OP>
static int band_launch(const char *domain, BandArgs a)
{
	typedef typename BandOut<T, OP>::type OUT;
	if (!on_unit(a.out, a.out_stride, sizeof(OUT))) {
		error(domain, "rows must start on whole elements");
		return -1;
	}
	for (int i = 0; i < a.n; i++)
		if (a.src[i].in && !on_unit(a.src[i].in, a.src[i].stride, sizeof(T))) {
			error(domain, "rows must start on whole elements");
			return -1;
		}
	constexpr int NE = POINTWISE_GROUP / (int) sizeof(OUT);
	bool streams = !logic_no_stream();
	if (streams) {
		// rows that follow one another without a gap on every side are one long row of width * height pels (as
		// pointwise_join_rows; the pels stay whole)
		BandArgs j = a;
		const int width = a.elems / a.out_bands;
		bool gapless = a.height > 1 && a.out_stride == (long long) a.elems * (int) sizeof(OUT);
		long long widest = (long long) a.elems * a.height * (long long) sizeof(OUT);
		for (int i = 0; i < a.n && gapless; i++) {
			const BandSource &s = a.src[i];
			const long long row = (long long) s.width * s.pel_elems * (long long) sizeof(T);
			gapless = !s.in || (s.width == width && s.height == a.height && s.stride == row);
			widest = row * a.height > widest ? row * a.height : widest;
		}
		if (a.height == 1 || (gapless && widest < (1LL << 31))) {
			j.elems = a.elems * a.height;
			j.height = 1;
			j.out_stride = 0;
			for (int i = 0; i < a.n; i++) {
				j.src[i].width *= a.height;
				j.src[i].height = 1;
				j.src[i].stride = 0;
			}
		}
		const long long groups = ((long long) j.elems + NE - 1) / NE;
		streams = on_unit(j.out, j.out_stride, 4) && groups * j.height < (1LL << 31);
		if (streams) {
			a = j;
			a.groups = (int) groups;
		}
	}
	if (streams) {
		if constexpr (OP == BAND_JOIN) {
			if (!band_pels_takes<T>(a))
				band_stream_launch<T, OP, 0>(a);
		}
		else {
			// the dword loads want the source's rows on dwords too
			const int b = on_unit(a.src[0].in, a.src[0].stride, 4) ? a.src[0].pel_elems : 0;
			switch (b) {
			case 2: band_stream_launch<T, OP, 2>(a); break;
			case 3: band_stream_launch<T, OP, 3>(a); break;
			case 4: band_stream_launch<T, OP, 4>(a); break;
			default: band_stream_launch<T, OP, 0>(a); break;
			}
		}
	}
	else {
		const int bx = (a.elems + POINTWISE_THREADS - 1) / POINTWISE_THREADS;
		dim3 grid(bx, pointwise_rows_grid(bx, a.height), 1);
		Gate gate("logic_band_general");
		hipLaunchKernelGGL((band_general_kernel<T, OP>), grid, dim3(POINTWISE_THREADS, 1, 1), 0, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

template <int OP>
static int band_by_format(const char *domain, int format, const BandArgs &a)
{
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR: return band_launch<u8, OP>(domain, a);
	case VIPS_HIP_FORMAT_CHAR: return band_launch<s8, OP>(domain, a);
	case VIPS_HIP_FORMAT_USHORT: return band_launch<u16, OP>(domain, a);
	case VIPS_HIP_FORMAT_SHORT: return band_launch<s16, OP>(domain, a);
	case VIPS_HIP_FORMAT_UINT: return band_launch<u32, OP>(domain, a);
	case VIPS_HIP_FORMAT_INT: return band_launch<s32, OP>(domain, a);
	case VIPS_HIP_FORMAT_FLOAT: return band_launch<f32, OP>(domain, a);
	case VIPS_HIP_FORMAT_DOUBLE: return band_launch<f64, OP>(domain, a);
	default:
		error(domain, "no kernel for format %d", format);
		return -1;
	}
}

int band_run(const char *domain, int op, int format, BandArgs a)
{
	if (a.elems < 1 || a.height < 1 || a.out_bands < 1 || a.elems % a.out_bands || a.n < 1 || a.n > BAND_MAX_SOURCES) {
		error(domain, "bad image size");
		return -1;
	}
	const int es = format_sizeof(format);
	long long widest = (long long) a.elems * (es > 4 ? es : 4);
	for (int i = 0; i < a.n; i++) {
		const long long row = (long long) a.src[i].width * a.src[i].pel_elems * es;
		widest = row > widest ? row : widest;
	}
	if (widest >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	switch (op) {
	case BAND_JOIN:
		// bandjoin.c:86-131 copies bytes: one kernel an element size
		switch (es) {
		case 1: return band_launch<u8, BAND_JOIN>(domain, a);
		case 2: return band_launch<u16, BAND_JOIN>(domain, a);
		case 4: return band_launch<u32, BAND_JOIN>(domain, a);
		case 8: return band_launch<u64, BAND_JOIN>(domain, a);
		default: break;
		}
		break;
	case BAND_MEAN: return band_by_format<BAND_MEAN>(domain, format, a);
	case BAND_AND: return band_by_format<BAND_AND>(domain, format, a);
	case BAND_OR: return band_by_format<BAND_OR>(domain, format, a);
	case BAND_EOR: return band_by_format<BAND_EOR>(domain, format, a);
	default: break;
	}
	error(domain, "no kernel for operation %d on format %d", op, format);
	return -1;
}

int logic_tile(int what)
{
	switch (what) {
	case 0: return POINTWISE_THREADS;
	case 1: return POINTWISE_GROUP;
	case 2: return POINTWISE_GRID_BLOCKS;
	default: return 0;
	}
}

} // namespace vh
