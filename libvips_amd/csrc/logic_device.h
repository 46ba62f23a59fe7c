// The expressions of vips_relational / vips_relational_const and vips_boolean / vips_boolean_const (arithmetic/relational.c,
// boolean.c) for one element, as device functions: logic.hip makes its kernels of them, and regions.hip's countlines takes
// the comparison vips_moreeq_const makes from here, so that every format thresholds as the reference's chain does.
#ifndef VH_LOGIC_DEVICE_H
#define VH_LOGIC_DEVICE_H

#include "pointwise.h"

namespace vh {

// ---------------------------------------------------------------- the reference's expressions

template <int FAMILY, typename IN>
struct LogicOut {
	typedef u8 type; // relational.c:214-217: uchar whatever the input
};
template <typename IN>
struct LogicOut<LOGIC_BOOLEAN, IN> {
	// boolean.c:253-256: integer formats keep their format, float and double give int
	typedef typename std::conditional<std::is_floating_point<IN>::value, s32, IN>::type type;
};

template <int OP, typename A>
VH_DEV bool logic_compare(A l, A r)
{
	if constexpr (OP == RELATIONAL_EQUAL)
		return l == r;
	else if constexpr (OP == RELATIONAL_NOTEQ)
		return l != r;
	else if constexpr (OP == RELATIONAL_LESS)
		return l < r;
	else if constexpr (OP == RELATIONAL_LESSEQ)
		return l <= r;
	else if constexpr (OP == RELATIONAL_MORE)
		return l > r;
	else
		return l >= r;
}

// One output element.  l: the pel; r: the other image's (two images) ; (ci, cd) element b of c_int / c_double
// (constants); is_int: unaryconst.c:108-113 and relational.c:528-529.
template <int FAMILY, int OP, bool CONST, typename IN>
VH_DEV typename LogicOut<FAMILY, IN>::type logic_elem(IN l, IN r, bool is_int, int ci, double cd)
{
	typedef typename LogicOut<FAMILY, IN>::type OUT;
	constexpr bool in_float = std::is_floating_point<IN>::value;
	if constexpr (FAMILY == LOGIC_RELATIONAL) {
		if constexpr (!CONST) {
			// RLOOP, relational.c:92-101: (left[x] ROP right[x]) ? 255 : 0 on two values of one type
			return logic_compare<OP, IN>(l, r) ? 255 : 0;
		}
		else {
			if constexpr (!in_float) {
				if (is_int) {
					// RLOOPCI, relational.c:472-481: p[i] OP c[b] with an int c -- the usual conversions: a uint pel
					// makes the constant unsigned, every other pel is promoted to int
					if constexpr (std::is_same<IN, u32>::value)
						return logic_compare<OP, u32>(l, (u32) ci) ? 255 : 0;
					else
						return logic_compare<OP, s32>((s32) l, ci) ? 255 : 0;
				}
			}
			// RLOOPCF, relational.c:483-492: p[i] OP c[b] with a double c
			return logic_compare<OP, f64>((f64) l, cd) ? 255 : 0;
		}
	}
	else if constexpr (CONST) {
		// LOOPC / FLOOPC, boolean.c:499-519: ((unsigned int) p[i]) OP c[b], an int c: unsigned arithmetic, the right
		// shift logical, stored to the pel's type (int for float and double)
		u32 p;
		if constexpr (in_float)
			p = (u32) cvt_i32(l);
		else
			p = (u32) l;
		if constexpr (OP == BOOLEAN_AND)
			return (OUT) (p & (u32) ci);
		else if constexpr (OP == BOOLEAN_OR)
			return (OUT) (p | (u32) ci);
		else if constexpr (OP == BOOLEAN_EOR)
			return (OUT) (p ^ (u32) ci);
		else if constexpr (OP == BOOLEAN_LSHIFT)
			return (OUT) (p << ci);
		else
			return (OUT) (p >> ci);
	}
	else {
		// LOOP / FLOOP / FNLOOP, boolean.c:96-115, :150-158: left[x] OP right[x] after the promotion to int (float and
		// double: (int) left[x] OP (int) right[x]); the left shift of signed formats is VIPS_LSHIFT_INT, an unsigned
		// shift, and that is what the left shift of the promoted unsigned ones is too; the right shift of signed
		// formats is arithmetic
		u32 a, b;
		if constexpr (in_float) {
			a = (u32) cvt_i32(l);
			b = (u32) cvt_i32(r);
		}
		else {
			a = (u32) l;
			b = (u32) r;
		}
		if constexpr (OP == BOOLEAN_AND)
			return (OUT) (a & b);
		else if constexpr (OP == BOOLEAN_OR)
			return (OUT) (a | b);
		else if constexpr (OP == BOOLEAN_EOR)
			return (OUT) (a ^ b);
		else if constexpr (OP == BOOLEAN_LSHIFT)
			return (OUT) (a << b);
		else if constexpr (std::is_unsigned<IN>::value)
			return (OUT) (a >> b);
		else
			return (OUT) ((s32) a >> b);
	}
}

} // namespace vh

#endif // VH_LOGIC_DEVICE_H
