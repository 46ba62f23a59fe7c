// vips_sum (arithmetic/sum.c:56-140) and vips_bandrank (conversion/bandrank.c:75-237) over 1 .. 16 images of one
// format on the device (gfx950), ONE launch an operation: the images' base pointers and strides are the kernel's
// arguments (staged to LDS, where a lane picks image i), no bandjoin or embed is made.
//
//   sum        accumulated in the OUTPUT type (uint for the unsigned formats, int for the signed ones, float, double),
//              image after image in index order: float order is the reference's, uint wraps (and so does int, which
//              the reference leaves undefined).
//   bandrank   index 0 and index n - 1 are the reference's FIND_MIN and FIND_MAX loops restated (bandrank.c:75-105):
//              a NaN in the first image stays, a NaN later never wins.  Any other index is the index-th smallest, found
//              by counting: the value whose rank -- the values below it, and the equal ones of earlier images -- is
//              the index; for values without NaN that is what the reference's insertion sort leaves at sort[index].
//
//   nary_stream<OP, IN, OUT>    images of the output's bands and size with rows that start on dwords on every side.
//                               A lane takes 16 bytes of an OUTPUT row at a time and folds image after image into its
//                               registers (sum, min, max: one global_store_dwordx4 a group); for the other indices it
//                               takes one dword (two of a double image), because it has to hold every image's share
//                               at once to count.  The groups of every row are dealt to the lanes as one sequence, rows
//                               without gaps are one row, a ragged last group goes element by element.
//   nary_general<OP, IN, OUT>   one output element a lane: a one-band image against n bands (indexed by pel), images of
//                               different sizes (zero outside an image's own rectangle), rows that start anywhere.  It
//                               defines correctness; VIPS_HIP_NO_NARY_STREAM sends everything to it.
#include "pointwise.h"

namespace vh {

// the sources from the kernel's arguments to LDS: thread i brings source i, picked by selects with constant indices (a
// by-value array indexed at run time would be copied to scratch)
VH_DEV void nary_sources(const NaryArgs &a, NarySource *src)
{
	const int t = tid();
	NarySource v = a.src[0];
#pragma unroll
	for (int i = 1; i < NARY_IMAGES; i++)
		if (t == i)
			v = a.src[i];
	if (t < NARY_IMAGES)
		src[t] = v;
	barrier();
}

// how image 0 starts an accumulator and how a later image is folded in
template <int OP, typename IN, typename OUT>
VH_DEV OUT nary_first(IN v)
{
	return (OUT) v; // sum.c:64, bandrank.c:78, :94
}
template <int OP, typename IN, typename OUT>
VH_DEV OUT nary_fold(OUT acc, IN v)
{
	if constexpr (OP == NARY_SUM) {
		// sum.c:66: sum += p[i][x] in OUT (unsigned arithmetic for both integer types: the same bits, nothing undefined)
		if constexpr (std::is_floating_point<OUT>::value)
			return acc + (OUT) v;
		else
			return (OUT) ((u32) acc + (u32) (OUT) v);
	}
	else if constexpr (OP == NARY_MIN)
		return v < acc ? v : acc; // bandrank.c:99-100
	else
		return v > acc ? v : acc; // bandrank.c:83-84
}

// One output element from the n values get(0) .. get(n - 1).
template <int OP, typename IN, typename OUT, typename Get>
VH_DEV OUT nary_elem(int n, int index, Get get)
{
	if constexpr (OP != NARY_RANK) {
		OUT acc = nary_first<OP, IN, OUT>(get(0));
		for (int i = 1; i < n; i++)
			acc = nary_fold<OP, IN, OUT>(acc, get(i));
		return acc;
	}
	else {
		// the index-th smallest: value i's rank is the number of values below it plus the equal ones before it
		IN r = get(0);
		for (int i = 0; i < n; i++) {
			const IN vi = get(i);
			int rank = 0;
			for (int j = 0; j < n; j++) {
				const IN vj = get(j);
				rank += j < i ? vj <= vi : vj < vi;
			}
			r = rank == index ? vi : r;
		}
		return r;
	}
}

template <int OP, typename IN, typename OUT>
__global__ void __launch_bounds__(POINTWISE_THREADS)
nary_general_kernel(NaryArgs a)
{
	__shared__ NarySource src[NARY_IMAGES];
	nary_sources(a, src);
	const int e = (int) blockIdx.x * POINTWISE_THREADS + (int) threadIdx.x;
	if (e >= a.elems)
		return;
	const int pel = e / a.bands;
	for (int y = (int) blockIdx.y; y < a.height; y += (int) gridDim.y) {
		const auto get = [&](int i) {
			const NarySource s = src[i];
			if (pel >= s.width || y >= s.height)
				return (IN) 0;
			return ((const IN *) (s.in + (long long) y * s.stride))[s.bands == 1 ? pel : e];
		};
		((OUT *) (a.out + (long long) y * a.out_stride))[e] = nary_elem<OP, IN, OUT>(a.n, a.index, get);
	}
}

// element i (a constant once the loops are unrolled) into the OD cleared dwords of a group of the output
template <typename T, int OD>
VH_DEV void nary_put(unsigned int (&w)[OD], int i, T v)
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

// bytes of the output a lane of the stream kernel makes at a time
template <int OP, typename OUT>
constexpr int nary_group()
{
	return OP == NARY_RANK ? (sizeof(OUT) > 4 ? (int) sizeof(OUT) : 4) : POINTWISE_GROUP;
}

template <int OP, typename IN, typename OUT>
__global__ void __launch_bounds__(POINTWISE_THREADS)
nary_stream_kernel(NaryArgs a)
{
	constexpr int GROUP = nary_group<OP, OUT>();
	constexpr int NE = GROUP / (int) sizeof(OUT);
	constexpr int ND = NE * (int) sizeof(IN) / 4; // dwords of an image's share of a group
	constexpr int OD = GROUP / 4;
	__shared__ NarySource src[NARY_IMAGES];
	nary_sources(a, src);
	const unsigned int total = (unsigned int) a.groups * (unsigned int) a.height;
	for (unsigned int at = (unsigned int) blockIdx.x * POINTWISE_THREADS + (unsigned int) threadIdx.x; at < total; at += (unsigned int) gridDim.x * POINTWISE_THREADS) {
		const int y = (int) (at / (unsigned int) a.groups);
		const int g = (int) (at - (unsigned int) y * (unsigned int) a.groups);
		const int e0 = g * NE;
		const int left = min(NE, a.elems - e0); // < NE: the row's ragged end
		const unsigned long long orow = (unsigned long long) a.out + (unsigned long long) y * a.out_stride;
		const unsigned int off = (unsigned int) e0 * (unsigned int) sizeof(IN);
		if (left == NE) {
			unsigned int w[OD];
#pragma unroll
			for (int k = 0; k < OD; k++)
				w[k] = 0;
			if constexpr (OP != NARY_RANK) {
				OUT acc[NE];
#pragma unroll
				for (int k = 0; k < NE; k++)
					acc[k] = (OUT) 0;
				for (int i = 0; i < a.n; i++) {
					const NarySource s = src[i];
					unsigned int d[ND];
					group_load<ND>(gptr_in_of((unsigned long long) s.in + (unsigned long long) y * s.stride), off, d);
#pragma unroll
					for (int k = 0; k < NE; k++) {
						const IN v = group_take<IN, ND>(d, k);
						acc[k] = i == 0 ? nary_first<OP, IN, OUT>(v) : nary_fold<OP, IN, OUT>(acc[k], v);
					}
				}
#pragma unroll
				for (int k = 0; k < NE; k++)
					nary_put<OUT, OD>(w, k, acc[k]);
				gstore_dwords<OD>(gptr_out_of(orow) + (unsigned int) g * GROUP, w);
			}
			else {
				// every image's share in registers: the loops are unrolled to the most images there can be, so that
				// every index is a constant
				unsigned int d[NARY_IMAGES][ND];
#pragma unroll
				for (int i = 0; i < NARY_IMAGES; i++)
					if (i < a.n) {
						const NarySource s = src[i];
						group_load<ND>(gptr_in_of((unsigned long long) s.in + (unsigned long long) y * s.stride), off, d[i]);
					}
#pragma unroll
				for (int k = 0; k < NE; k++) {
					IN r = group_take<IN, ND>(d[0], k);
#pragma unroll
					for (int i = 0; i < NARY_IMAGES; i++)
						if (i < a.n) {
							const IN vi = group_take<IN, ND>(d[i], k);
							int rank = 0;
#pragma unroll
							for (int j = 0; j < NARY_IMAGES; j++)
								if (j != i && j < a.n) {
									const IN vj = group_take<IN, ND>(d[j], k);
									rank += j < i ? vj <= vi : vj < vi;
								}
							r = rank == a.index ? vi : r;
						}
					nary_put<OUT, OD>(w, k, r);
				}
				gstore_dwords<OD>(gptr_out_of(orow) + (unsigned int) g * GROUP, w);
			}
		}
		else {
			for (int k = 0; k < left; k++) {
				const int e = e0 + k;
				const auto get = [&](int i) {
					const NarySource s = src[i];
					return ((const IN *) (s.in + (long long) y * s.stride))[e];
				};
				((OUT *) orow)[e] = nary_elem<OP, IN, OUT>(a.n, a.index, get);
			}
		}
	}
}

// ---------------------------------------------------------------- dispatch

// The stream kernel takes this call: then its rows are joined and `groups` is set.
template <int OP, typename IN, typename OUT>
static bool nary_streams(NaryArgs &a)
{
	if (getenv("VIPS_HIP_NO_NARY_STREAM"))
		return false;
	const int width = a.elems / a.bands;
	for (int i = 0; i < a.n; i++)
		if (a.src[i].bands != a.bands || a.src[i].width < width || a.src[i].height < a.height)
			return false;
	NaryArgs joined = a;
	// (one row is nothing away from a next one: its stride must not count in the alignment)
	bool gapless = a.height > 1 && a.out_stride == (long long) a.elems * (long long) sizeof(OUT) &&
		(long long) a.elems * a.height * (long long) (sizeof(OUT) > sizeof(IN) ? sizeof(OUT) : sizeof(IN)) < (1LL << 31);
	for (int i = 0; i < a.n && gapless; i++)
		gapless = a.src[i].width == width && a.src[i].stride == (long long) a.elems * (long long) sizeof(IN);
	if (gapless) {
		joined.elems = a.elems * a.height;
		joined.height = 1;
	}
	if (joined.height == 1) {
		joined.out_stride = 0;
		for (int i = 0; i < a.n; i++)
			joined.src[i].stride = 0;
	}
	constexpr int NE = nary_group<OP, OUT>() / (int) sizeof(OUT);
	const long long groups = ((long long) joined.elems + NE - 1) / NE;
	// rows that start on dwords on every side; the kernel numbers the groups in 32 bits
	if (!on_unit(joined.out, joined.out_stride, 4) || groups * joined.height >= (1LL << 31))
		return false;
	for (int i = 0; i < a.n; i++)
		if (!on_unit(joined.src[i].in, joined.src[i].stride, 4))
			return false;
	a = joined;
	a.groups = (int) groups;
	return true;
}

template <int OP, typename IN, typename OUT>
static int nary_launch(const char *domain, NaryArgs a)
{
	if (!on_unit(a.out, a.out_stride, sizeof(OUT))) {
		error(domain, "rows must start on whole elements");
		return -1;
	}
	for (int i = 0; i < a.n; i++)
		if (!on_unit(a.src[i].in, a.src[i].stride, sizeof(IN))) {
			error(domain, "rows must start on whole elements");
			return -1;
		}
	dim3 block(POINTWISE_THREADS, 1, 1);
	if (nary_streams<OP, IN, OUT>(a)) {
		Gate gate("nary_stream");
		hipLaunchKernelGGL((nary_stream_kernel<OP, IN, OUT>), pointwise_stream_grid((long long) a.groups * a.height), block, 0, stream(), a);
	}
	else {
		const int bx = (a.elems + POINTWISE_THREADS - 1) / POINTWISE_THREADS;
		dim3 grid(bx, pointwise_rows_grid(bx, a.height), 1);
		Gate gate("nary_general");
		hipLaunchKernelGGL((nary_general_kernel<OP, IN, OUT>), grid, block, 0, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

int nary_tile(int what)
{
	switch (what) {
	case 0: return POINTWISE_THREADS;
	case 1: return POINTWISE_GRID_BLOCKS;
	case 2: return nary_group<NARY_SUM, u32>();
	case 3: return nary_group<NARY_RANK, u8>();
	case 4: return nary_group<NARY_RANK, f64>();
	default: return 0;
	}
}

// Everything has been checked (ops_nary.cpp).
int nary_run(const char *domain, int op, int format, NaryArgs a)
{
	if (a.n < 1 || a.n > NARY_IMAGES || a.elems < 1 || a.height < 1 || a.bands < 1 || a.elems % a.bands || op < 0 || op >= NARY_LAST ||
		(op == NARY_RANK && (a.index < 0 || a.index >= a.n))) {
		error(domain, "bad arguments");
		return -1;
	}
	if ((long long) a.elems * 8 >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	for (int i = 0; i < a.n; i++)
		if (!a.src[i].in || a.src[i].width < 1 || a.src[i].height < 1 || (a.src[i].bands != 1 && a.src[i].bands != a.bands) ||
			(long long) a.src[i].width * a.src[i].bands * 8 >= (1LL << 31)) {
			error(domain, "bad image %d", i);
			return -1;
		}
#define F(name) VIPS_HIP_FORMAT_##name
#define GO(OP, FI, TI, TO) \
	if (op == OP && format == F(FI)) \
		return nary_launch<OP, TI, TO>(domain, a);
	// sum.c:137-140
	GO(NARY_SUM, UCHAR, u8, u32) GO(NARY_SUM, CHAR, s8, s32) GO(NARY_SUM, USHORT, u16, u32) GO(NARY_SUM, SHORT, s16, s32)
	GO(NARY_SUM, UINT, u32, u32) GO(NARY_SUM, INT, s32, s32) GO(NARY_SUM, FLOAT, f32, f32) GO(NARY_SUM, DOUBLE, f64, f64)
#define SAME(OP) \
	GO(OP, UCHAR, u8, u8) GO(OP, CHAR, s8, s8) GO(OP, USHORT, u16, u16) GO(OP, SHORT, s16, s16) GO(OP, UINT, u32, u32) \
	GO(OP, INT, s32, s32) GO(OP, FLOAT, f32, f32) GO(OP, DOUBLE, f64, f64)
	SAME(NARY_MIN)
	SAME(NARY_MAX)
	SAME(NARY_RANK)
#undef SAME
#undef GO
#undef F
	error(domain, "no kernel for operation %d on format %d", op, format);
	return -1;
}

} // namespace vh
