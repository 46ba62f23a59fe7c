// vips_linear, vips_invert, vips_abs (arithmetic/linear.c, invert.c, abs.c), vips_add, vips_subtract, vips_multiply,
// vips_divide (add.c, subtract.c, multiply.c, divide.c), vips_round, vips_sign, vips_clamp, vips_minpair, vips_maxpair,
// vips_remainder, vips_remainder_const (round.c, sign.c, clamp.c, minpair.c, maxpair.c, remainder.c) and the scan of
// vips_stats (stats.c) on the device (gfx950).
//
// The pointwise operations are ONE launch that writes every output byte once: pointwise.h's stream kernel
// (arith_stream) where the rows start on dwords on every side and every operand has the output's shape, its one-element-
// a-lane kernel (arith_general) for the rest and for everything under VIPS_HIP_NO_ARITH_STREAM.  This file gives them
// the expressions (arith_elem), the policy (ArithOp: vips_linear's band vectors are the constants staged to LDS) and
// the table of formats (arith_run).
//
// The arithmetic is the reference's, expression by expression (arith_elem below cites each); the file is compiled with
// -ffp-contract=off, so multiplies and adds stay separate as in the reference's baseline x86-64 code, and float
// division is the correctly rounded quotient (__fdiv_rn / __ddiv_rn).
//
// vips_stats: one read-only pass.
//
//   stats_stream<T, B>   B = 1 .. 4 bands, rows that start on dwords.  A lane takes 16 / sizeof(T) pels at a time -- B
//                        groups of 16 bytes, so the band of every element of what it holds is known when the kernel is
//                        compiled and the per-band accumulators stay in registers -- grid-strided over the image's
//                        groups with a capped grid.  Per band: sum and sum of squares (64-bit integers for the integer
//                        formats: exact; doubles for float), the extremes and the raster index of the FIRST pel that
//                        holds each.  NaN never compares, so it enters neither extreme (stats.c:268-277) but does enter
//                        the sums.  Lanes meet in LDS in a tree of fixed shape, thread 0 writes the block's partial to
//                        a slab, the host merges the slab in index order: no floating atomics, the order depends on
//                        the image's geometry alone.
//   stats_general<T>     any band count and any row start: block (x, band), one element a lane and step.
#include "pointwise.h"

namespace vh {

constexpr int STATS_GRID_BLOCKS = 1024; // four a CU, as hist_rects

// ---------------------------------------------------------------- the reference's expressions

// VIPS_FCLIP(0, t, 255) = fmax(0, fmin(255, t)) and the conversion to uchar (linear.c:277, :292): fmin gives 255 for a
// NaN, as this comparison does; what is left lies in 0 .. 255 and the conversion truncates
template <typename F>
VH_DEV unsigned char arith_clip_u8(F t)
{
	F c = t < (F) 255 ? t : (F) 255;
	c = c > (F) 0 ? c : (F) 0;
	return (unsigned char) cvt_i32(c);
}

template <typename T>
VH_DEV T arith_negate(T x)
{
	if constexpr (std::is_floating_point<T>::value)
		return -x;
	else
		return (T) (0u - (unsigned int) x); // (wraps, as the reference's stores do)
}

// One output element.  x, y: the operands; (a1, b1) vips_linear's constants as floats for its single-element loops,
// (ak, bk) element k of a_ready / b_ready.
template <int OP, typename IN, typename OUT>
VH_DEV OUT arith_elem(IN x, IN y, bool single, float a1, float b1, double ak, double bk)
{
	constexpr bool in_float = std::is_floating_point<IN>::value;
	if constexpr (OP == ARITH_LINEAR) {
		if constexpr (std::is_same<OUT, unsigned char>::value) {
			if (single) {
				// LOOP1uc, linear.c:266-279: float a1, b1; float t = a1 * p[x] + b1 -- for a double image the
				// product and the sum are double (the usual conversions) and t rounds them
				if constexpr (std::is_same<IN, double>::value)
					return arith_clip_u8<float>((float) ((double) a1 * x + (double) b1));
				else
					return arith_clip_u8<float>(a1 * (float) x + b1);
			}
			// LOOPNuc, linear.c:283-294: double t = a[k] * p[i] + b[k]
			return arith_clip_u8<double>(ak * (double) x + bk);
		}
		else if constexpr (std::is_same<OUT, float>::value) {
			// LOOP1, linear.c:213-223: OUT a1 = a[0]; q = a1 * (OUT) p + b1, float arithmetic
			if (single)
				return a1 * (float) x + b1;
			// LOOPN, linear.c:227-235: a[k] * (OUT) p[i] + b[k] -- the pel rounded to float, the arithmetic double,
			// the store rounds
			return (float) (ak * (double) (float) x + bk);
		}
		else
			return ak * (double) x + bk; // LOOP1 and LOOPN of a double image are the same double expression
	}
	else if constexpr (OP == ARITH_INVERT) {
		// invert.c:71-87: L - p for the unsigned formats, -1 * p for the others (an exact sign change for every
		// number)
		if constexpr (std::is_unsigned<IN>::value)
			return (OUT) ((IN) ~(IN) 0 - x);
		else
			return arith_negate(x);
	}
	else if constexpr (OP == ARITH_ABS) {
		// abs.c:100-120: p < 0 ? 0 - p : p; fabs(); the unsigned formats are a copy (abs.c:88-90)
		if constexpr (std::is_same<IN, float>::value)
			return __builtin_fabsf(x);
		else if constexpr (std::is_same<IN, double>::value)
			return __builtin_fabs(x);
		else if constexpr (std::is_unsigned<IN>::value)
			return x;
		else
			return x < 0 ? arith_negate(x) : x;
	}
	else if constexpr (OP == ARITH_DIVIDE) {
		// divide.c:122-131: right == 0 ? 0 : (OUT) left / (OUT) right
		if constexpr (std::is_same<OUT, double>::value)
			return y == (IN) 0 ? 0.0 : __ddiv_rn((double) x, (double) y);
		else
			return y == (IN) 0 ? 0.0f : __fdiv_rn((float) x, (float) y);
	}
	else if constexpr (in_float) {
		return OP == ARITH_ADD ? x + y : OP == ARITH_SUBTRACT ? x - y : x * y;
	}
	else {
		// add.c:70-92, subtract.c:70-92, multiply.c:102-126: the sum, difference or product of the two values in a
		// type that holds it (int64 for int images), stored to OUT; modulo 2^32 that is this
		const unsigned int l = (unsigned int) x, r = (unsigned int) y;
		return (OUT) (OP == ARITH_ADD ? l + r : OP == ARITH_SUBTRACT ? l - r : l * r);
	}
}

// a double to an integer format whose range holds it after truncation: the store's conversion of round.c, clamp.c
template <typename T>
VH_DEV T arith_store(double v)
{
	if constexpr (std::is_same<T, float>::value)
		return (float) v;
	else if constexpr (std::is_same<T, double>::value)
		return v;
	else {
		// (a value outside the format's range: the reference's conversion is undefined; here it saturates)
		constexpr double lo = std::is_unsigned<T>::value ? 0.0 : -(double) (1ull << (8 * sizeof(T) - 1));
		constexpr double hi = std::is_unsigned<T>::value ? (double) ((1ull << (8 * sizeof(T) - 1)) - 1) * 2.0 + 1.0 : (double) ((1ull << (8 * sizeof(T) - 1)) - 1);
		const double c = v < lo ? lo : v > hi ? hi : v;
		return cvt_to<T, double>(c);
	}
}

// fmin / fmax (minpair.c:73, maxpair.c:73): a NaN loses to a number.  Of zeros of opposite sign the reference's libm
// returns one or the other by the order of its arguments; here -0 is below +0 in either order (IEEE 754's minimum and
// maximum): equal operands differ in nothing but that sign, which min sets and max clears.
template <bool MAX, typename F>
VH_DEV F arith_fpair(F x, F y)
{
	typedef typename std::conditional<sizeof(F) == 4, unsigned int, u64>::type Bits;
	if (x != x)
		return y;
	if (y != y)
		return x;
	if (x == y) {
		const Bits bx = __builtin_bit_cast(Bits, x), by = __builtin_bit_cast(Bits, y);
		return __builtin_bit_cast(F, MAX ? (Bits) (bx & by) : (Bits) (bx | by));
	}
	return (MAX ? x > y : x < y) ? x : y;
}

// One output element of round, sign, clamp, minpair, maxpair, remainder and remainder_const.  x, y: the operands;
// round: ROUND_*; (ak, bk): clamp's min and max, or remainder_const's c_int[k] in ak.
template <int OP, typename IN, typename OUT>
VH_DEV OUT arith2_elem(IN x, IN y, int round, double ak, double bk)
{
	constexpr bool in_float = std::is_floating_point<IN>::value;
	if constexpr (OP == ARITH_ROUND) {
		// round.c:87-141: rint / ceil / floor in the image's own type; integer images are a copy (round.c:77-79)
		if constexpr (std::is_same<IN, float>::value)
			return round == ROUND_RINT ? __builtin_rintf(x) : round == ROUND_CEIL ? __builtin_ceilf(x) : __builtin_floorf(x);
		else if constexpr (std::is_same<IN, double>::value)
			return round == ROUND_RINT ? __builtin_rint(x) : round == ROUND_CEIL ? __builtin_ceil(x) : __builtin_floor(x);
		else
			return x;
	}
	else if constexpr (OP == ARITH_SIGN) {
		// sign.c:86-102: a NaN is neither > 0 nor == 0
		return x > (IN) 0 ? (OUT) 1 : x == (IN) 0 ? (OUT) 0 : (OUT) -1;
	}
	else if constexpr (OP == ARITH_CLAMP) {
		// clamp.c:62-69: VIPS_MAX(min, VIPS_MIN(max, p)) with double bounds, then the store's conversion; the
		// comparisons let a NaN pel through
		const double v = (double) x;
		const double inner = bk < v ? bk : v;
		return arith_store<OUT>(ak > inner ? ak : inner);
	}
	else if constexpr (OP == ARITH_MINPAIR || OP == ARITH_MAXPAIR) {
		// minpair.c:56-74, maxpair.c:56-74
		if constexpr (in_float)
			return arith_fpair<OP == ARITH_MAXPAIR, IN>(x, y);
		else
			return (OP == ARITH_MAXPAIR ? x > y : x < y) ? x : y;
	}
	else if constexpr (in_float) {
		// remainder.c:106-118, :286-299: b ? a - b * floor(a / b) : -1 in double, the store rounds
		const double a = (double) x;
		double b;
		if constexpr (OP == ARITH_REMAINDER)
			b = (double) y;
		else
			b = ak;
		return (OUT) (b != 0.0 ? a - __dmul_rn(b, __builtin_floor(__ddiv_rn(a, b))) : -1.0);
	}
	else if constexpr (OP == ARITH_REMAINDER) {
		// remainder.c:94-102: p2 ? p1 % p2 : -1 (the format's maximum for the unsigned ones).  A divisor of -1
		// leaves 0 whatever the dividend: the reference traps on INT_MIN % -1, here that is 0 too
		if (y == (IN) 0)
			return (OUT) -1;
		if constexpr (std::is_signed<IN>::value)
			return y == (IN) -1 ? (OUT) 0 : (OUT) ((int) x % (int) y);
		else
			return (OUT) ((unsigned int) x % (unsigned int) y);
	}
	else {
		// remainder.c:273-282: c[b] ? p % c[b] : -1 with c an int: the usual conversions make c unsigned for a uint
		// image and the pel an int for every other
		const int c = cvt_i32(ak);
		if (c == 0)
			return (OUT) -1;
		if constexpr (std::is_same<IN, unsigned int>::value)
			return x % (unsigned int) c;
		else
			return c == -1 ? (OUT) 0 : (OUT) ((int) x % c);
	}
}

// ---------------------------------------------------------------- the policy

// vips_linear's band vectors from the kernel's arguments to LDS: thread i brings element i, picked by selects with
// constant indices (a by-value array indexed at run time would be copied to scratch)
VH_DEV void arith_constants(const ArithArgs &a, double *ca, double *cb)
{
	const int t = tid();
	double va = 0.0, vb = 0.0;
#pragma unroll
	for (int i = 0; i < ARITH_MAX_VECTOR; i++) {
		va = t == i ? a.a[i] : va;
		vb = t == i ? a.b[i] : vb;
	}
	if (t < ARITH_MAX_VECTOR) {
		ca[t] = va;
		cb[t] = vb;
	}
	barrier();
}

template <int OP, typename IN_, typename OUT_>
struct ArithOp {
	typedef IN_ IN;
	typedef OUT_ OUT;
	typedef ArithArgs Args;
	typedef double CA, CB;
	static constexpr int MAX_VECTOR = ARITH_MAX_VECTOR;
	static constexpr bool binary = arith_binary(OP);
	// (clamp's two bounds and remainder_const's c_int reach elem() the way vips_linear's vectors do)
	static constexpr bool constants = OP == ARITH_LINEAR || OP == ARITH_CLAMP || OP == ARITH_REMAINDER_CONST;
	VH_DEV void stage(const ArithArgs &a, double *ca, double *cb) { arith_constants(a, ca, cb); }
	VH_DEV OUT elem(const ArithArgs &a, IN l, IN r, double ak, double bk)
	{
		if constexpr (OP >= ARITH_ROUND)
			return arith2_elem<OP, IN, OUT>(l, r, a.round, ak, bk);
		else
			return arith_elem<OP, IN, OUT>(l, r, a.single != 0, a.a1, a.b1f, ak, bk);
	}
};

int arith_tile(int what)
{
	switch (what) {
	case 0: return POINTWISE_THREADS;
	case 1: return POINTWISE_GROUP;
	case 2: return POINTWISE_GRID_BLOCKS;
	case 3: return STATS_GRID_BLOCKS;
	default: return 0;
	}
}

int arith_run(const char *domain, int op, int in_format, int out_format, ArithArgs a)
{
	if (a.elems < 1 || a.height < 1 || a.bands < 1 || a.elems % a.bands) {
		error(domain, "bad image size");
		return -1;
	}
	const long long widest = format_sizeof(in_format) > format_sizeof(out_format) ? format_sizeof(in_format) : format_sizeof(out_format);
	if ((long long) a.elems * widest >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	if ((op == ARITH_LINEAR || op == ARITH_REMAINDER_CONST) && !a.single && a.bands > ARITH_MAX_VECTOR) {
		error(domain, "vectors of more than %d elements are outside the HIP path", ARITH_MAX_VECTOR);
		return -1;
	}
#define F(name) VIPS_HIP_FORMAT_##name
#define GO(OP, FI, TI, FO, TO) \
	if (op == OP && in_format == F(FI) && out_format == F(FO)) \
		return pointwise_launch<ArithOp<OP, TI, TO>>(domain, a, "arith_stream", "arith_general", "VIPS_HIP_NO_ARITH_STREAM");
	// linear.c:425-428, and `uchar`
	GO(ARITH_LINEAR, UCHAR, u8, FLOAT, f32) GO(ARITH_LINEAR, CHAR, s8, FLOAT, f32) GO(ARITH_LINEAR, USHORT, u16, FLOAT, f32)
	GO(ARITH_LINEAR, SHORT, s16, FLOAT, f32) GO(ARITH_LINEAR, UINT, u32, FLOAT, f32) GO(ARITH_LINEAR, INT, s32, FLOAT, f32)
	GO(ARITH_LINEAR, FLOAT, f32, FLOAT, f32) GO(ARITH_LINEAR, DOUBLE, f64, DOUBLE, f64)
	GO(ARITH_LINEAR, UCHAR, u8, UCHAR, u8) GO(ARITH_LINEAR, CHAR, s8, UCHAR, u8) GO(ARITH_LINEAR, USHORT, u16, UCHAR, u8)
	GO(ARITH_LINEAR, SHORT, s16, UCHAR, u8) GO(ARITH_LINEAR, UINT, u32, UCHAR, u8) GO(ARITH_LINEAR, INT, s32, UCHAR, u8)
	GO(ARITH_LINEAR, FLOAT, f32, UCHAR, u8) GO(ARITH_LINEAR, DOUBLE, f64, UCHAR, u8)
	// invert.c:166-169, abs.c:188-191
#define SAME(OP) \
	GO(OP, UCHAR, u8, UCHAR, u8) GO(OP, CHAR, s8, CHAR, s8) GO(OP, USHORT, u16, USHORT, u16) GO(OP, SHORT, s16, SHORT, s16) \
	GO(OP, UINT, u32, UINT, u32) GO(OP, INT, s32, INT, s32) GO(OP, FLOAT, f32, FLOAT, f32) GO(OP, DOUBLE, f64, DOUBLE, f64)
	SAME(ARITH_INVERT)
	SAME(ARITH_ABS)
	// round.c:157-160, clamp.c:139-142, minpair.c:139-142, maxpair.c:139-142, remainder.c:175-178 (both forms)
	SAME(ARITH_ROUND)
	SAME(ARITH_CLAMP)
	SAME(ARITH_MINPAIR)
	SAME(ARITH_MAXPAIR)
	SAME(ARITH_REMAINDER)
	SAME(ARITH_REMAINDER_CONST)
#undef SAME
	// sign.c:162-165
	GO(ARITH_SIGN, UCHAR, u8, CHAR, s8) GO(ARITH_SIGN, CHAR, s8, CHAR, s8) GO(ARITH_SIGN, USHORT, u16, CHAR, s8)
	GO(ARITH_SIGN, SHORT, s16, CHAR, s8) GO(ARITH_SIGN, UINT, u32, CHAR, s8) GO(ARITH_SIGN, INT, s32, CHAR, s8)
	GO(ARITH_SIGN, FLOAT, f32, CHAR, s8) GO(ARITH_SIGN, DOUBLE, f64, CHAR, s8)
	// add.c:180-183, multiply.c:197-200
#define SUM(OP) \
	GO(OP, UCHAR, u8, USHORT, u16) GO(OP, CHAR, s8, SHORT, s16) GO(OP, USHORT, u16, UINT, u32) GO(OP, SHORT, s16, INT, s32) \
	GO(OP, UINT, u32, UINT, u32) GO(OP, INT, s32, INT, s32) GO(OP, FLOAT, f32, FLOAT, f32) GO(OP, DOUBLE, f64, DOUBLE, f64)
	SUM(ARITH_ADD)
	SUM(ARITH_MULTIPLY)
#undef SUM
	// subtract.c:176-179
	GO(ARITH_SUBTRACT, UCHAR, u8, SHORT, s16) GO(ARITH_SUBTRACT, CHAR, s8, SHORT, s16) GO(ARITH_SUBTRACT, USHORT, u16, INT, s32)
	GO(ARITH_SUBTRACT, SHORT, s16, INT, s32) GO(ARITH_SUBTRACT, UINT, u32, INT, s32) GO(ARITH_SUBTRACT, INT, s32, INT, s32)
	GO(ARITH_SUBTRACT, FLOAT, f32, FLOAT, f32) GO(ARITH_SUBTRACT, DOUBLE, f64, DOUBLE, f64)
	// divide.c:199-202
	GO(ARITH_DIVIDE, UCHAR, u8, FLOAT, f32) GO(ARITH_DIVIDE, CHAR, s8, FLOAT, f32) GO(ARITH_DIVIDE, USHORT, u16, FLOAT, f32)
	GO(ARITH_DIVIDE, SHORT, s16, FLOAT, f32) GO(ARITH_DIVIDE, UINT, u32, FLOAT, f32) GO(ARITH_DIVIDE, INT, s32, FLOAT, f32)
	GO(ARITH_DIVIDE, FLOAT, f32, FLOAT, f32) GO(ARITH_DIVIDE, DOUBLE, f64, DOUBLE, f64)
#undef GO
#undef F
	error(domain, "no kernel for operation %d from format %d to format %d", op, in_format, out_format);
	return -1;
}

// ---------------------------------------------------------------- stats

struct StatsArgs {
	const unsigned char *in;
	StatsPartial *out;
	long long stride; // bytes
	int width, height, bands;
	int groups; // (stream kernel) groups of 16 / sizeof(T) pels of a row, the ragged one included
};

template <typename T>
struct StatsSums {
	typedef long long Sum;
	typedef unsigned long long Sum2;
};
template <>
struct StatsSums<float> {
	typedef double Sum;
	typedef double Sum2;
};

// stats.c:247-330 for one band: sum += value; sum2 += (double) value * (double) value; the extremes by > and <, which a
// NaN never passes.  (The reference starts its extremes at the first value it meets, NaN or not: which value that is
// depends on how its threads cut the image up, so a NaN there is no contract; here a NaN is never an extreme.)
template <typename T>
struct StatsAcc {
	typename StatsSums<T>::Sum sum;
	typename StatsSums<T>::Sum2 sum2;
	T mn, mx;
	unsigned int imn, imx;

	__device__ __forceinline__ void clear()
	{
		sum = 0;
		sum2 = 0;
		mn = mx = (T) 0;
		imn = imx = STATS_NONE;
	}
	// (a lane meets its pels in raster order: the strict comparisons keep the first of equals)
	__device__ __forceinline__ void take(T v, unsigned int index)
	{
		sum += v;
		if constexpr (std::is_floating_point<T>::value)
			sum2 += (double) v * (double) v;
		else if constexpr (sizeof(T) == 4) // (uint, int: vips_min and vips_max only, the sums are not used)
			sum2 += (unsigned long long) (long long) v * (unsigned long long) (long long) v;
		else
			sum2 += (unsigned long long) ((long long) v * (long long) v);
		if (imx == STATS_NONE ? v == v : v > mx) {
			mx = v;
			imx = index;
		}
		if (imn == STATS_NONE ? v == v : v < mn) {
			mn = v;
			imn = index;
		}
	}
};

template <typename T>
VH_DEV unsigned int stats_bits(T v)
{
	if constexpr (std::is_floating_point<T>::value)
		return __builtin_bit_cast(unsigned int, v);
	else
		return (unsigned int) (int) v;
}

// the block's lanes meet in LDS, pairs at half the distance each step; thread 0 writes the partial
template <typename T>
VH_DEV void stats_block_reduce(const StatsAcc<T> &acc, StatsPartial *dst)
{
	typedef typename StatsSums<T>::Sum Sum;
	typedef typename StatsSums<T>::Sum2 Sum2;
	__shared__ Sum s_sum[POINTWISE_THREADS];
	__shared__ Sum2 s_sum2[POINTWISE_THREADS];
	__shared__ T s_mn[POINTWISE_THREADS], s_mx[POINTWISE_THREADS];
	__shared__ unsigned int s_imn[POINTWISE_THREADS], s_imx[POINTWISE_THREADS];
	const int t = tid();
	barrier(); // (the band before this one has been read)
	s_sum[t] = acc.sum;
	s_sum2[t] = acc.sum2;
	s_mn[t] = acc.mn;
	s_mx[t] = acc.mx;
	s_imn[t] = acc.imn;
	s_imx[t] = acc.imx;
	barrier();
	for (int s = POINTWISE_THREADS / 2; s > 0; s >>= 1) {
		if (t < s) {
			const int o = t + s;
			s_sum[t] += s_sum[o];
			s_sum2[t] += s_sum2[o];
			// the smaller value, of equals the one met first in raster order
			if (s_imn[o] != STATS_NONE && (s_imn[t] == STATS_NONE || s_mn[o] < s_mn[t] || (s_mn[o] == s_mn[t] && s_imn[o] < s_imn[t]))) {
				s_mn[t] = s_mn[o];
				s_imn[t] = s_imn[o];
			}
			if (s_imx[o] != STATS_NONE && (s_imx[t] == STATS_NONE || s_mx[o] > s_mx[t] || (s_mx[o] == s_mx[t] && s_imx[o] < s_imx[t]))) {
				s_mx[t] = s_mx[o];
				s_imx[t] = s_imx[o];
			}
		}
		barrier();
	}
	if (t == 0) {
		StatsPartial p;
		if constexpr (std::is_floating_point<T>::value) {
			p.sum = __builtin_bit_cast(unsigned long long, s_sum[0]);
			p.sum2 = __builtin_bit_cast(unsigned long long, s_sum2[0]);
		}
		else {
			p.sum = (unsigned long long) s_sum[0];
			p.sum2 = s_sum2[0];
		}
		p.mn = stats_bits<T>(s_mn[0]);
		p.mx = stats_bits<T>(s_mx[0]);
		p.imn = s_imn[0];
		p.imx = s_imx[0];
		*dst = p;
	}
}

template <typename T, int B>
__global__ void __launch_bounds__(POINTWISE_THREADS)
stats_stream_kernel(StatsArgs a)
{
	constexpr int NP = POINTWISE_GROUP / (int) sizeof(T); // pels a lane takes at a time: B groups of 16 bytes
	StatsAcc<T> acc[B];
#pragma unroll
	for (int b = 0; b < B; b++)
		acc[b].clear();
	const unsigned int total = (unsigned int) a.groups * (unsigned int) a.height;
	for (unsigned int at = (unsigned int) blockIdx.x * POINTWISE_THREADS + (unsigned int) threadIdx.x; at < total; at += (unsigned int) gridDim.x * POINTWISE_THREADS) {
		const int y = (int) (at / (unsigned int) a.groups);
		const int g = (int) (at - (unsigned int) y * (unsigned int) a.groups);
		const int p0 = g * NP;
		const int n = min(NP, a.width - p0);
		const unsigned long long row = (unsigned long long) a.in + (unsigned long long) y * a.stride;
		const unsigned int index = (unsigned int) y * (unsigned int) a.width + (unsigned int) p0;
		if (n == NP) {
			unsigned int d[4 * B];
			group_load<4 * B>(gptr_in_of(row), (unsigned int) g * (unsigned int) (POINTWISE_GROUP * B), d);
#pragma unroll
			for (int j = 0; j < NP * B; j++)
				acc[j % B].take(group_take<T, 4 * B>(d, j), index + (unsigned int) (j / B));
		}
		else {
			for (int j = 0; j < n; j++) {
#pragma unroll
				for (int b = 0; b < B; b++)
					acc[b].take(((const T *) row)[(p0 + j) * B + b], index + (unsigned int) j);
			}
		}
	}
#pragma unroll
	for (int b = 0; b < B; b++)
		stats_block_reduce<T>(acc[b], a.out + (size_t) blockIdx.x * B + b);
}

template <typename T>
__global__ void __launch_bounds__(POINTWISE_THREADS)
stats_general_kernel(StatsArgs a)
{
	const int band = (int) blockIdx.y;
	StatsAcc<T> acc;
	acc.clear();
	const unsigned int total = (unsigned int) a.width * (unsigned int) a.height;
	for (unsigned int at = (unsigned int) blockIdx.x * POINTWISE_THREADS + (unsigned int) threadIdx.x; at < total; at += (unsigned int) gridDim.x * POINTWISE_THREADS) {
		const unsigned int y = at / (unsigned int) a.width, x = at - y * (unsigned int) a.width;
		acc.take(((const T *) (a.in + (long long) y * a.stride))[(long long) x * a.bands + band], at);
	}
	stats_block_reduce<T>(acc, a.out + (size_t) blockIdx.x * a.bands + band);
}

// rows that follow one another without a gap are one long row of width * height pels: the raster index of a pel is
// the same, and an image streams whatever its width
static bool stats_joined(const _VipsHipImage *in)
{
	const long long row = (long long) in->width * in->bands * format_sizeof(in->format);
	return (long long) in->stride == row && row * in->height < (1LL << 31);
}

static bool stats_stream_ok(const _VipsHipImage *in)
{
	if (getenv("VIPS_HIP_NO_ARITH_STREAM") || in->bands > 4)
		return false;
	return ((uintptr_t) in->data | (uintptr_t) (stats_joined(in) ? 0 : in->stride)) % 4 == 0;
}

static int stats_groups(const _VipsHipImage *in)
{
	const int np = POINTWISE_GROUP / format_sizeof(in->format);
	return ((stats_joined(in) ? in->width * in->height : in->width) + np - 1) / np;
}

int stats_blocks(const _VipsHipImage *in)
{
	long long blocks;
	if (stats_stream_ok(in))
		blocks = ((long long) stats_groups(in) * (stats_joined(in) ? 1 : in->height) + POINTWISE_THREADS - 1) / POINTWISE_THREADS;
	else
		blocks = ((long long) in->width * in->height + POINTWISE_THREADS - 1) / POINTWISE_THREADS;
	const int cap = stats_stream_ok(in) ? STATS_GRID_BLOCKS : STATS_GRID_BLOCKS / (in->bands < STATS_GRID_BLOCKS ? in->bands : STATS_GRID_BLOCKS);
	blocks = blocks > cap ? cap : blocks;
	return (int) (blocks < 1 ? 1 : blocks);
}

template <typename T>
static int stats_launch(const char *domain, const _VipsHipImage *in, StatsArgs a)
{
	const int blocks = stats_blocks(in);
	dim3 block(POINTWISE_THREADS, 1, 1);
	if (stats_stream_ok(in)) {
		a.groups = stats_groups(in);
		if (stats_joined(in)) {
			a.width *= a.height;
			a.height = 1;
		}
		dim3 grid(blocks, 1, 1);
		Gate gate("stats_stream");
		switch (in->bands) {
		case 1: hipLaunchKernelGGL((stats_stream_kernel<T, 1>), grid, block, 0, stream(), a); break;
		case 2: hipLaunchKernelGGL((stats_stream_kernel<T, 2>), grid, block, 0, stream(), a); break;
		case 3: hipLaunchKernelGGL((stats_stream_kernel<T, 3>), grid, block, 0, stream(), a); break;
		default: hipLaunchKernelGGL((stats_stream_kernel<T, 4>), grid, block, 0, stream(), a); break;
		}
	}
	else {
		dim3 grid(blocks, in->bands, 1);
		Gate gate("stats_general");
		hipLaunchKernelGGL((stats_general_kernel<T>), grid, block, 0, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

// Everything has been checked (ops_arith.cpp).
int stats_run(const char *domain, const _VipsHipImage *in, StatsPartial *slab)
{
	// (the kernels number pels in 32 bits, STATS_NONE excluded)
	if (in->width < 1 || in->height < 1 || in->bands < 1 || in->bands > 65535 || (long long) in->width * in->height >= (1LL << 31) ||
		(long long) in->width * in->bands * format_sizeof(in->format) >= (1LL << 31)) {
		error(domain, "image too large");
		return -1;
	}
	if (((uintptr_t) in->data | (uintptr_t) in->stride) % (uintptr_t) format_sizeof(in->format)) {
		error(domain, "rows must start on whole elements");
		return -1;
	}
	StatsArgs a = {};
	a.in = (const unsigned char *) in->data;
	a.out = slab;
	a.stride = (long long) in->stride;
	a.width = in->width;
	a.height = in->height;
	a.bands = in->bands;
	switch (in->format) {
	case VIPS_HIP_FORMAT_UCHAR: return stats_launch<u8>(domain, in, a);
	case VIPS_HIP_FORMAT_CHAR: return stats_launch<s8>(domain, in, a);
	case VIPS_HIP_FORMAT_USHORT: return stats_launch<u16>(domain, in, a);
	case VIPS_HIP_FORMAT_SHORT: return stats_launch<s16>(domain, in, a);
	case VIPS_HIP_FORMAT_UINT: return stats_launch<u32>(domain, in, a);
	case VIPS_HIP_FORMAT_INT: return stats_launch<s32>(domain, in, a);
	case VIPS_HIP_FORMAT_FLOAT: return stats_launch<f32>(domain, in, a);
	default:
		error(domain, "no kernel for format %d", in->format);
		return -1;
	}
}

} // namespace vh
