// The streaming scaffold of the pointwise families (arith.hip, logic.hip; trim.hip and canvas.hip take its helpers
// and grids): what a lane does with the 16-byte groups of a row, and how the host decides between the two kernels.
//
//   pointwise_stream<Op>    lanes on consecutive 16-byte groups of an OUTPUT row: 16 / sizeof(OUT) elements, whose
//                           operands are 16 * sizeof(IN) / sizeof(OUT) bytes of the input row -- 4 to 128, always
//                           whole dwords at a dword offset, so with rows that start on dwords on every side the lane
//                           loads them as aligned dwords (global_load_dwordx4 where there are four) and stores one
//                           global_store_dwordx4.  The rows' groups are dealt to the lanes as one sequence; a row's
//                           ragged last group goes element by element inside the same launch.  Per-band constants lie
//                           in LDS and are picked by (element index) mod bands.
//   pointwise_general<Op>   one element a lane: defines correctness and takes what the stream declines -- rows that
//                           do not start on dwords, a one-band operand against n bands (indexed by pel), operands
//                           of different sizes (zero outside an operand's rectangle: vips__sizealike's black embed
//                           at (0, 0), arithmetic.c:139-171) -- and everything under the family's VIPS_HIP_NO_*_STREAM.
//
// Op is a family's policy: the types IN, OUT and Args (a PointwiseGeom and the family's constants, the kernel's one
// argument), `binary` (there is a right-hand operand), `constants` (two tables of MAX_VECTOR entries of CA and CB are
// staged to LDS by stage()), and elem(a, l, r, ca, cb): one output element from the operands and the constants picked
// for its band.
#ifndef VH_POINTWISE_H
#define VH_POINTWISE_H

#include "gcn.h"
#include "internal.h"
#include "kernel_stmt.h"

#include <cstdint>
#include <cstdlib>
#include <type_traits>

namespace vh {

constexpr int POINTWISE_THREADS = 256;
constexpr int POINTWISE_GROUP = 16;            // bytes of the output a lane makes at a time
constexpr int POINTWISE_GRID_BLOCKS = 256 * 8; // of a stream launch

typedef unsigned char u8;
typedef signed char s8;
typedef unsigned short u16;
typedef short s16;
typedef unsigned int u32;
typedef int s32;
typedef float f32;
typedef double f64;
typedef unsigned long long u64;

// ---------------------------------------------------------------- registers <-> elements

// element i (a constant once the loops are unrolled) of the dwords of a group
template <typename T, int ND>
VH_DEV T group_take(const unsigned int (&d)[ND], int i)
{
	if constexpr (sizeof(T) == 1)
		return (T) (d[i >> 2] >> (8 * (i & 3)));
	else if constexpr (sizeof(T) == 2)
		return (T) (d[i >> 1] >> (16 * (i & 1)));
	else if constexpr (sizeof(T) == 4)
		return __builtin_bit_cast(T, d[i]);
	else
		return __builtin_bit_cast(T, (u64) d[2 * i] | ((u64) d[2 * i + 1] << 32));
}

template <typename T>
VH_DEV void group_put(unsigned int (&w)[4], int i, T v)
{
	if constexpr (sizeof(T) == 1)
		w[i >> 2] |= (unsigned int) (u8) v << (8 * (i & 3));
	else if constexpr (sizeof(T) == 2)
		w[i >> 1] |= (unsigned int) (u16) v << (16 * (i & 1));
	else if constexpr (sizeof(T) == 4)
		w[i] = __builtin_bit_cast(unsigned int, v);
	else {
		const u64 bits = __builtin_bit_cast(u64, v);
		w[2 * i] = (unsigned int) bits;
		w[2 * i + 1] = (unsigned int) (bits >> 32);
	}
}

// ND dwords (1, 2 or a multiple of 4) at a dword-aligned offset
template <int ND>
VH_DEV void group_load(gptr_in base, unsigned int off, unsigned int (&d)[ND])
{
	if constexpr (ND < 4)
		gload_dwords<ND>(base, off, d);
	else {
#pragma unroll
		for (int q = 0; q < ND / 4; q++) {
			unsigned int t[4];
			gload128(base, off + 16u * (unsigned int) q, t);
#pragma unroll
			for (int i = 0; i < 4; i++)
				d[4 * q + i] = t[i];
		}
	}
}

// ---------------------------------------------------------------- one element a lane

template <typename Op>
__global__ void __launch_bounds__(POINTWISE_THREADS)
pointwise_general_kernel(typename Op::Args a)
{
	typedef typename Op::IN IN;
	typedef typename Op::OUT OUT;
	__shared__ typename Op::CA ca[Op::MAX_VECTOR];
	__shared__ typename Op::CB cb[Op::MAX_VECTOR];
	if constexpr (Op::constants)
		Op::stage(a, ca, cb);
	const int e = (int) blockIdx.x * POINTWISE_THREADS + (int) threadIdx.x;
	if (e >= a.elems)
		return;
	const int pel = e / a.bands, k = e - pel * a.bands;
	const int i1 = a.b1 == 1 ? pel : e, i2 = a.b2 == 1 ? pel : e;
	typename Op::CA ak = 0;
	typename Op::CB bk = 0;
	if constexpr (Op::constants) {
		ak = ca[a.single ? 0 : k];
		bk = cb[a.single ? 0 : k];
	}
	for (int y = (int) blockIdx.y; y < a.height; y += (int) gridDim.y) {
		IN l = (IN) 0, r = (IN) 0;
		if (pel < a.w1 && y < a.h1)
			l = ((const IN *) (a.in + (long long) y * a.in_stride))[i1];
		if constexpr (Op::binary)
			if (pel < a.w2 && y < a.h2)
				r = ((const IN *) (a.in2 + (long long) y * a.in2_stride))[i2];
		((OUT *) (a.out + (long long) y * a.out_stride))[e] = Op::elem(a, l, r, ak, bk);
	}
}

// ---------------------------------------------------------------- 16 bytes of the output a lane

template <typename Op>
__global__ void __launch_bounds__(POINTWISE_THREADS)
pointwise_stream_kernel(typename Op::Args a)
{
	typedef typename Op::IN IN;
	typedef typename Op::OUT OUT;
	constexpr int NE = POINTWISE_GROUP / (int) sizeof(OUT);
	constexpr int ND = NE * (int) sizeof(IN) / 4; // dwords of an operand's group
	__shared__ typename Op::CA ca[Op::MAX_VECTOR];
	__shared__ typename Op::CB cb[Op::MAX_VECTOR];
	if constexpr (Op::constants)
		Op::stage(a, ca, cb);
	const bool vector = Op::constants && !a.single;
	typename Op::CA a0 = 0;
	typename Op::CB b0 = 0;
	if constexpr (Op::constants) {
		a0 = ca[0];
		b0 = cb[0];
	}
	const unsigned int total = (unsigned int) a.groups * (unsigned int) a.height;
	for (unsigned int at = (unsigned int) blockIdx.x * POINTWISE_THREADS + (unsigned int) threadIdx.x; at < total; at += (unsigned int) gridDim.x * POINTWISE_THREADS) {
		const int y = (int) (at / (unsigned int) a.groups);
		const int g = (int) (at - (unsigned int) y * (unsigned int) a.groups);
		const int e0 = g * NE;
		const int n = min(NE, a.elems - e0); // < NE: the row's ragged end
		const unsigned long long irow = (unsigned long long) a.in + (unsigned long long) y * a.in_stride;
		const unsigned long long irow2 = (unsigned long long) a.in2 + (unsigned long long) y * a.in2_stride;
		const unsigned long long orow = (unsigned long long) a.out + (unsigned long long) y * a.out_stride;
		int k = vector ? e0 % a.bands : 0;
		if (n == NE) {
			unsigned int d[ND], d2[ND], w[4] = { 0, 0, 0, 0 };
			group_load<ND>(gptr_in_of(irow), (unsigned int) e0 * (unsigned int) sizeof(IN), d);
			if constexpr (Op::binary)
				group_load<ND>(gptr_in_of(irow2), (unsigned int) e0 * (unsigned int) sizeof(IN), d2);
#pragma unroll
			for (int i = 0; i < NE; i++) {
				const IN l = group_take<IN, ND>(d, i);
				IN r = (IN) 0;
				if constexpr (Op::binary)
					r = group_take<IN, ND>(d2, i);
				typename Op::CA ak = a0;
				typename Op::CB bk = b0;
				if constexpr (Op::constants)
					if (vector) {
						ak = ca[k];
						bk = cb[k];
						k = k + 1 == a.bands ? 0 : k + 1;
					}
				group_put<OUT>(w, i, Op::elem(a, l, r, ak, bk));
			}
			gstore128(gptr_out_of(orow) + (unsigned int) g * POINTWISE_GROUP, w);
		}
		else {
			for (int i = 0; i < n; i++) {
				const IN l = ((const IN *) irow)[e0 + i];
				IN r = (IN) 0;
				if constexpr (Op::binary)
					r = ((const IN *) irow2)[e0 + i];
				typename Op::CA ak = a0;
				typename Op::CB bk = b0;
				if constexpr (Op::constants)
					if (vector) {
						ak = ca[k];
						bk = cb[k];
						k = k + 1 == a.bands ? 0 : k + 1;
					}
				((OUT *) orow)[e0 + i] = Op::elem(a, l, r, ak, bk);
			}
		}
	}
}

// ---------------------------------------------------------------- dispatch

static int pointwise_rows_grid(int blocks_x, int rows)
{
	// enough blocks to fill the part, rows dealt round-robin over grid.y
	int gy = (POINTWISE_GRID_BLOCKS + blocks_x - 1) / blocks_x;
	gy = gy < 1 ? 1 : gy;
	return gy > rows ? rows : gy;
}

// enough blocks to fill the part, the rest of a lane's units in turns
static dim3 pointwise_stream_grid(long long units)
{
	const long long blocks = (units + POINTWISE_THREADS - 1) / POINTWISE_THREADS;
	return dim3((unsigned int) (blocks < POINTWISE_GRID_BLOCKS ? blocks : POINTWISE_GRID_BLOCKS), 1, 1);
}

// every row starts on a multiple of `unit`
static bool on_unit(const void *p, long long stride, uintptr_t unit)
{
	return ((uintptr_t) p | (uintptr_t) stride) % unit == 0;
}

static bool pointwise_on_units(const PointwiseGeom &g, bool binary, uintptr_t in_unit, uintptr_t out_unit)
{
	return on_unit(g.in, g.in_stride, in_unit) && (!binary || on_unit(g.in2, g.in2_stride, in_unit)) && on_unit(g.out, g.out_stride, out_unit);
}

// every operand as wide, as tall and of as many bands as the output: element e of a row is element e of every side
static bool pointwise_same_shape(const PointwiseGeom &g, bool binary)
{
	const int width = g.elems / g.bands;
	if (g.b1 != g.bands || g.w1 < width || g.h1 < g.height)
		return false;
	return !binary || (g.b2 == g.bands && g.w2 >= width && g.h2 >= g.height);
}

// Rows that follow one another without a gap on every side are one long row (it starts on a multiple of `bands`
// elements wherever a row did, so the band of an element does not change): whole images then stream whatever their
// width, and the ragged end is the image's, not every row's.
static void pointwise_join_rows(PointwiseGeom &g, bool binary, int in_es, int out_es)
{
	const long long elems = (long long) g.elems * g.height;
	// (one row is nothing away from a next one: its stride must not count in the alignment)
	if (g.height == 1)
		g.in_stride = g.in2_stride = g.out_stride = 0;
	if (g.height > 1 && g.in_stride == (long long) g.elems * in_es && g.out_stride == (long long) g.elems * out_es &&
		(!binary || g.in2_stride == g.in_stride) && g.w1 == g.elems / g.bands && (!binary || g.w2 == g.w1) &&
		elems * (in_es > out_es ? in_es : out_es) < (1LL << 31)) {
		g.elems = (int) elems;
		g.w1 = g.w2 = g.elems / g.bands;
		g.h1 = g.h2 = g.height = 1;
		// (... nor the joined rows' own length)
		g.in_stride = g.in2_stride = g.out_stride = 0;
	}
}

// The stream kernel takes this geometry: then its rows are joined and `groups` is set.  `off_switch` names the
// environment variable that sends everything to the general kernel.
static bool pointwise_streams(PointwiseGeom &g, bool binary, int in_es, int out_es, const char *off_switch)
{
	if (getenv(off_switch) || !pointwise_same_shape(g, binary))
		return false;
	PointwiseGeom joined = g;
	pointwise_join_rows(joined, binary, in_es, out_es);
	const int ne = POINTWISE_GROUP / out_es;
	const long long groups = ((long long) joined.elems + ne - 1) / ne;
	// rows that start on dwords on every side; the kernel numbers the groups in 32 bits
	if (!pointwise_on_units(joined, binary, 4, 4) || groups * joined.height >= (1LL << 31))
		return false;
	g = joined;
	g.groups = (int) groups;
	return true;
}

template <typename Op>
static int pointwise_launch(const char *domain, typename Op::Args a, const char *stream_gate, const char *general_gate, const char *off_switch)
{
	if (!pointwise_on_units(a, Op::binary, sizeof(typename Op::IN), sizeof(typename Op::OUT))) {
		error(domain, "rows must start on whole elements");
		return -1;
	}
	dim3 block(POINTWISE_THREADS, 1, 1);
	if (pointwise_streams(a, Op::binary, (int) sizeof(typename Op::IN), (int) sizeof(typename Op::OUT), off_switch)) {
		Gate gate(stream_gate);
		hipLaunchKernelGGL((pointwise_stream_kernel<Op>), pointwise_stream_grid((long long) a.groups * a.height), block, 0, stream(), a);
	}
	else {
		const int bx = (a.elems + POINTWISE_THREADS - 1) / POINTWISE_THREADS;
		dim3 grid(bx, pointwise_rows_grid(bx, a.height), 1);
		Gate gate(general_gate);
		hipLaunchKernelGGL((pointwise_general_kernel<Op>), grid, block, 0, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

} // namespace vh

#endif // VH_POINTWISE_H
