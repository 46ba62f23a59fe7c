// vips_hist_find (arithmetic/hist_find.c) for uchar images on the device (gfx950): the histograms of up to six
// rectangles of one image in ONE launch -- what an iteration of vips_smartcrop's entropy search needs
// (conversion/smartcrop.c:129-173: left and right slice, then top and bottom slice for either outcome).
//
//   hist_rects<B>  B = 1 .. 4 bands.  Block (x, k) works on rectangle k.  A WAVE owns a row of the rectangle at a
//                  time (rows wave, wave + all the rectangle's waves, ...): lane l takes the 16 bytes at the row's
//                  first byte rounded DOWN to 16 bytes + 16 l (+ 1024 per further step).  A rectangle's rows start
//                  on any byte (a left offset in a 3-band image; a stride that is no multiple of 16): a group that
//                  lies wholly inside the row is one global_load_dwordx4, the group at either end goes byte by byte
//                  and only for the bytes inside -- nothing outside the rectangle is read.
//                  Every wave counts into a histogram of its own in LDS (256 x B counters, bin value * B + band:
//                  the order of the reference's output pels; 4 waves x 4 KB at most) with LDS atomic adds -- lanes
//                  of a wave do meet on a bin, waves do not.  After one barrier the block adds its four
//                  histograms and sends every NON-ZERO sum to the rectangle's counters in global memory with one
//                  integer atomic.  Integer sums do not depend on their order: the counts are exact and the same
//                  on every run.  The counters must be zero on entry.
//
//                  The launch is spread over 1 024 blocks, all rectangles together.
//
// Measured (an 8192 x 8192 x 3 image, inside the Infinity Cache): 0.067 ms on noise, 0.091 ms on a quiet
// picture -- the kernel is bound by the LDS atomics, and lanes that meet on a bin wait for one another.
#include "gcn.h"
#include "internal.h"
#include "kernel_stmt.h"

#include <cstdint>

namespace vh {

constexpr int HIST_THREADS = 256;
constexpr int HIST_WAVES = HIST_THREADS / 64;
constexpr int HIST_GROUP = 16;                // bytes a lane takes at a time
constexpr int HIST_WAVE_BYTES = 64 * HIST_GROUP; // ... a wave, of one row
constexpr int HIST_GRID_BLOCKS = 1024;        // of a launch, all rectangles together: four a CU

struct HistArgs {
	const unsigned char *in;
	unsigned int *out; // 256 * B counters per rectangle
	long long stride;  // bytes
	HistRect rect[HIST_MAX_RECTS];
};

template <int B>
__global__ void __launch_bounds__(HIST_THREADS)
hist_rects_kernel(HistArgs a)
{
	constexpr int BINS = 256 * B;
	__shared__ unsigned int bins[HIST_WAVES * BINS];
	const int tid = (int) threadIdx.x;
	const int lane = tid & 63;
	const int wave = wave_index();

	for (int i = tid; i < HIST_WAVES * BINS; i += HIST_THREADS)
		bins[i] = 0;
	__syncthreads();

	// (selects, not an index: a by-value array indexed at run time would be copied to scratch)
	const int k = (int) blockIdx.y;
	HistRect r = a.rect[0];
#pragma unroll
	for (int j = 1; j < HIST_MAX_RECTS; j++)
		if (k == j)
			r = a.rect[j];

	unsigned int *mine = bins + wave * BINS;
	const int rowbytes = r.width * B;
	const int all_waves = (int) gridDim.x * HIST_WAVES;
	for (int y = (int) blockIdx.x * HIST_WAVES + wave; y < r.height; y += all_waves) {
		const unsigned long long start = (unsigned long long) a.in + (unsigned long long) (r.top + y) * a.stride +
			(unsigned long long) r.left * B;
		const int sh = (int) (start & (HIST_GROUP - 1));
		const gptr_in base = gptr_in_of(start - sh);
		const int groups = (sh + rowbytes + HIST_GROUP - 1) / HIST_GROUP;
		for (int g = lane; g < groups; g += 64) {
			const int q0 = HIST_GROUP * g - sh; // where in the row the group's first byte is
			if (q0 >= 0 && q0 + HIST_GROUP <= rowbytes) {
				unsigned int w[4];
				gload128(base, (unsigned int) (HIST_GROUP * g), w);
				int band = q0 % B;
#pragma unroll
				for (int i = 0; i < HIST_GROUP; i++) {
					const unsigned int v = (w[i >> 2] >> (8 * (i & 3))) & 255u;
					atomicAdd(&mine[v * B + band], 1u);
					band = band + 1 == B ? 0 : band + 1;
				}
			}
			else {
				for (int i = 0; i < HIST_GROUP; i++) {
					const int q = q0 + i;
					if (q >= 0 && q < rowbytes) {
						const unsigned int v = gload8(base, (unsigned int) (HIST_GROUP * g + i));
						atomicAdd(&mine[v * B + q % B], 1u);
					}
				}
			}
		}
	}
	__syncthreads();

	unsigned int *out = a.out + (size_t) k * BINS;
	for (int i = tid; i < BINS; i += HIST_THREADS) {
		unsigned int sum = 0;
#pragma unroll
		for (int w = 0; w < HIST_WAVES; w++)
			sum += bins[w * BINS + i];
		if (sum)
			atomicAdd(&out[i], sum);
	}
}

int hist_rects(const char *domain, const _VipsHipImage *in, const HistRect *rects, int n, unsigned int *counters)
{
	if (!in || !rects || !counters) {
		error(domain, "null argument");
		return -1;
	}
	if (in->format != VIPS_HIP_FORMAT_UCHAR || in->bands < 1 || in->bands > 4) {
		error(domain, "histograms are of uchar images of 1 to 4 bands");
		return -1;
	}
	if (n < 1 || n > HIST_MAX_RECTS) {
		error(domain, "1 to %d rectangles a launch", HIST_MAX_RECTS);
		return -1;
	}
	// (the reference changes to double counters at 2^32 pels: hist_find.c:156-162)
	if ((long long) in->width * in->height >= (1LL << 31) || (long long) in->width * in->bands >= (1LL << 31) - 64) {
		error(domain, "image too large");
		return -1;
	}
	HistArgs a = {};
	a.in = (const unsigned char *) in->data;
	a.out = counters;
	a.stride = (long long) in->stride;
	int tallest = 1;
	for (int k = 0; k < n; k++) {
		const HistRect &r = rects[k];
		if (r.width <= 0 || r.height <= 0 || r.left < 0 || r.top < 0 || (long long) r.left + r.width > in->width ||
			(long long) r.top + r.height > in->height) {
			error(domain, "bad extract area");
			return -1;
		}
		a.rect[k] = r;
		tallest = r.height > tallest ? r.height : tallest;
	}
	int bx = (tallest + HIST_WAVES - 1) / HIST_WAVES;
	bx = bx > HIST_GRID_BLOCKS / n ? HIST_GRID_BLOCKS / n : bx;
	dim3 grid(bx, n, 1), block(HIST_THREADS, 1, 1);
	{
		Gate gate("hist_rects");
		switch (in->bands) {
		case 1: hipLaunchKernelGGL((hist_rects_kernel<1>), grid, block, 0, stream(), a); break;
		case 2: hipLaunchKernelGGL((hist_rects_kernel<2>), grid, block, 0, stream(), a); break;
		case 3: hipLaunchKernelGGL((hist_rects_kernel<3>), grid, block, 0, stream(), a); break;
		default: hipLaunchKernelGGL((hist_rects_kernel<4>), grid, block, 0, stream(), a); break;
		}
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

// ---- vips_maplut (histogram/maplut.c) of a uchar image
//
//   maplut_u8<ES>  ES = 1, 2, 4, 8 bytes a table entry.  The table -- up to 256 entries x 4 tables x 8 bytes -- is
//                  copied to LDS once a block; then, as above, a WAVE owns a row at a time and lane l the 16 input
//                  bytes at the row's first byte rounded down to 16 + 16 l: one global_load_dwordx4 inside the row,
//                  byte loads for the bytes inside at either end.  Every input byte is clipped to n - 1 (maplut.c's
//                  clp) and looked up; input element q of a row goes through table q % tables (one table: every
//                  element through it), or, a one-band image through `spread` tables, through each of them in turn.
//                  A lane's results are consecutive bytes of the output row: 4- and 8-byte entries are stored as
//                  dwords; 1- and 2-byte entries are gathered in a register pair and leave as whole dwords from the
//                  first 4-byte boundary on -- only what lies before it, and what is left at the end, goes entry by
//                  entry, and no two lanes ever write the same dword's bytes twice.

constexpr int MAPLUT_THREADS = 256;
constexpr int MAPLUT_WAVES = MAPLUT_THREADS / 64;
constexpr int MAPLUT_GRID_BLOCKS = 1024;

template <int ES>
struct MaplutOut {
	unsigned long long pos; // where the next byte goes
	unsigned long long acc;
	int held; // bytes in acc

	__device__ __forceinline__ void unit(unsigned int v)
	{
		if constexpr (ES == 1)
			gstore8(gptr_out_of(pos), (unsigned char) v);
		else
			gstore16(gptr_out_of(pos), (unsigned short) v);
		pos += ES;
	}
	__device__ __forceinline__ void put(const unsigned int (&v)[2])
	{
		if constexpr (ES >= 4) {
			gstore32(gptr_out_of(pos), v[0]);
			if constexpr (ES == 8)
				gstore32(gptr_out_of(pos + 4), v[1]);
			pos += ES;
		}
		else if (held == 0 && (pos & 3) != 0)
			unit(v[0]);
		else {
			acc |= (unsigned long long) v[0] << (8 * held);
			held += ES;
			if (held >= 4) {
				gstore32(gptr_out_of(pos), (unsigned int) acc);
				pos += 4;
				acc >>= 32;
				held -= 4;
			}
		}
	}
	__device__ __forceinline__ void flush()
	{
		if constexpr (ES < 4)
			for (; held > 0; held -= ES) {
				unit((unsigned int) acc & (ES == 1 ? 0xffu : 0xffffu));
				acc >>= 8 * ES;
			}
	}
};

template <int ES>
VH_DEV void maplut_entry(const unsigned int *table, unsigned int k, unsigned int (&v)[2])
{
	if constexpr (ES == 1)
		v[0] = (table[k >> 2] >> (8 * (k & 3))) & 0xffu;
	else if constexpr (ES == 2)
		v[0] = (table[k >> 1] >> (16 * (k & 1))) & 0xffffu;
	else if constexpr (ES == 4)
		v[0] = table[k];
	else {
		v[0] = table[2 * k];
		v[1] = table[2 * k + 1];
	}
}

template <int ES>
__global__ void __launch_bounds__(MAPLUT_THREADS)
maplut_kernel(MaplutArgs a)
{
	__shared__ unsigned int table[MAPLUT_TABLE_MAX / 4];
	const int tid = (int) threadIdx.x;
	const int lane = tid & 63;
	const int wave = wave_index();

	// (the table's block is whole dwords)
	const int table_dwords = (a.n * a.tables * ES + 3) / 4;
	for (int i = tid; i < table_dwords; i += MAPLUT_THREADS)
		table[i] = gload32(gptr_in_of((unsigned long long) a.table), 4u * (unsigned int) i);
	__syncthreads();

	const unsigned int clip = (unsigned int) a.n - 1u;
	const int all_waves = (int) gridDim.x * MAPLUT_WAVES;
	for (int y = (int) blockIdx.x * MAPLUT_WAVES + wave; y < a.height; y += all_waves) {
		const unsigned long long start = (unsigned long long) a.in + (unsigned long long) y * (unsigned long long) a.in_stride;
		const unsigned long long orow = (unsigned long long) a.out + (unsigned long long) y * (unsigned long long) a.out_stride;
		const int sh = (int) (start & (HIST_GROUP - 1));
		const gptr_in base = gptr_in_of(start - sh);
		const int groups = (sh + a.in_elems + HIST_GROUP - 1) / HIST_GROUP;
		for (int g = lane; g < groups; g += 64) {
			const int q0 = HIST_GROUP * g - sh; // where in the row the group's first byte is
			unsigned int w[4] = { 0, 0, 0, 0 };
			if (q0 >= 0 && q0 + HIST_GROUP <= a.in_elems)
				gload128(base, (unsigned int) (HIST_GROUP * g), w);
			else {
#pragma unroll
				for (int i = 0; i < HIST_GROUP; i++) {
					const int q = q0 + i;
					if (q >= 0 && q < a.in_elems)
						w[i >> 2] |= (unsigned int) gload8(base, (unsigned int) (HIST_GROUP * g + i)) << (8 * (i & 3));
				}
			}
			const int first = q0 < 0 ? 0 : q0; // the first element of the row this lane makes
			MaplutOut<ES> out = { orow + (unsigned long long) first * (unsigned long long) (a.spread * ES), 0, 0 };
			int z = a.tables > 1 && a.spread == 1 ? first % a.tables : 0;
#pragma unroll
			for (int i = 0; i < HIST_GROUP; i++) {
				const int q = q0 + i;
				if (q >= 0 && q < a.in_elems) {
					unsigned int v = (w[i >> 2] >> (8 * (i & 3))) & 255u;
					v = v > clip ? clip : v;
					unsigned int e[2];
					if (a.spread > 1) {
						for (int zz = 0; zz < a.spread; zz++) {
							maplut_entry<ES>(table, v * (unsigned int) a.tables + (unsigned int) zz, e);
							out.put(e);
						}
					}
					else {
						maplut_entry<ES>(table, v * (unsigned int) a.tables + (unsigned int) z, e);
						out.put(e);
						z = z + 1 >= a.tables ? 0 : z + 1;
					}
				}
			}
			out.flush();
		}
	}
}

template <int ES>
static int maplut_launch(const MaplutArgs &a)
{
	int bx = (a.height + MAPLUT_WAVES - 1) / MAPLUT_WAVES;
	bx = bx > MAPLUT_GRID_BLOCKS ? MAPLUT_GRID_BLOCKS : bx;
	{
		Gate gate("maplut_u8");
		hipLaunchKernelGGL((maplut_kernel<ES>), dim3(bx, 1, 1), dim3(MAPLUT_THREADS, 1, 1), 0, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

// Everything has been checked (ops_histogram.cpp).
int maplut_run(const char *domain, MaplutArgs a)
{
	if (a.n < 1 || a.n > 256 || a.tables < 1 || a.spread < 1 || (a.spread > 1 && a.spread != a.tables) ||
		(long long) a.n * a.tables * a.es > MAPLUT_TABLE_MAX) {
		error(domain, "a table of %d entries x %d bands x %d bytes: the kernel keeps up to %d bytes", a.n, a.tables, a.es, MAPLUT_TABLE_MAX);
		return -1;
	}
	if ((long long) a.in_elems * a.spread * a.es >= (1LL << 31) - 64) {
		error(domain, "image too large");
		return -1;
	}
	switch (a.es) {
	case 1: return maplut_launch<1>(a);
	case 2: return maplut_launch<2>(a);
	case 4: return maplut_launch<4>(a);
	case 8: return maplut_launch<8>(a);
	default:
		error(domain, "table entries of %d bytes", a.es);
		return -1;
	}
}

} // namespace vh

extern "C" {

// what the kernel takes at a time: 0 the bytes of a row a wave takes in a step, 1 the rows a block takes in a step,
// 2 / 3 the most blocks a histogram launch (all rectangles together) / a maplut launch has
int vips_hip_hist_step(int what)
{
	switch (what) {
	case 0: return vh::HIST_WAVE_BYTES;
	case 1: return vh::HIST_WAVES;
	case 2: return vh::HIST_GRID_BLOCKS;
	case 3: return vh::MAPLUT_GRID_BLOCKS;
	default: return 0;
	}
}

} // extern "C"
