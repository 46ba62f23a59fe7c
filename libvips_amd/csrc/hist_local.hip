// vips_hist_local (histogram/hist_local.c: local histogram equalisation, CLAHE with max_slope > 0) and vips_stdif
// (histogram/stdif.c: statistical differencing) for uchar images on the device (gfx950).  Both are sliding-window
// operations over the halo tile of nbhd_tile.h: output element (x, y, b) looks at the width x height window whose
// top-left is input pel (x - width / 2, y - height / 2), band b -- the embed the reference puts in front, a MIRROR for
// hist_local (hist_local.c:301-306), an edge copy for stdif (stdif.c:284-289) -- and at the pel itself, the "centre".
//
// hist_local: sum = how many window elements are <= the centre (CLAHE: with every bin clipped to max_slope and what
// was clipped spread evenly over the 256 bins, hist_local.c:211-238), out = 255 * sum / (width * height).
//
//   hist_local_count  max_slope 0 and width * height <= 64.  No histogram: the answer is a count of compares over the
//                     window in LDS, the way rank_select counts.  A block of 256 threads makes 256 elements x 8 rows,
//                     thread t owns column t.  width * height byte reads an element: cheaper than the sliding
//                     histogram's 2 height updates + half a scan up to about that size.
//   hist_local_slide  everything else, CLAHE always: the reference's own sliding histogram, one a LANE.  A block of 128
//                     threads makes 8 rows x (16 / bands) runs of 16 pels: lane (row, run, band) fills its histogram
//                     from the window of the run's first pel, then for every further pel takes one window column out
//                     and one in (2 height updates) and scans.
//
// The bins (MI355X_MICROARCH.md, LDS): 256 counters of 16 bits a lane, two to a dword -- 512 bytes a lane, 64 KB a
// block, which leaves 96 KB of the CU's 160 for the tile (8 + height - 1 rows) -- so width * height <= 65535.  Dword
// d of lane t lies at dword d * 128 + t: the bank of everything a lane touches is t mod 32, every access of a wave is
// conflict-free whatever the pixels are (lane-major bins would put a wave's 64 random values on random banks, about
// 3.5-way conflicts), and a scan is 128 ds_read_b32 at 2 LDS cycles each.  Updates are returnless LDS atomic adds of
// +-1 or +-0x10000 on the lane's OWN dwords: nothing contends (no other lane ever touches them); the atomic is there
// because a read-modify-write in registers is one LDS round trip after the other (the compiler cannot know that two
// bins differ), while ds_add_u32 without a result issues back to back.  A decrement never borrows (the element being
// removed was counted), an increment never carries (a bin holds at most width * height <= 65535).
// The scan works on both halves of a dword at once: v_pk_min_u16 clips, a 32-bit add accumulates (a half's sum is
// at most width * height: no carry).  Since the bins of a window add up to width * height, what CLAHE clipped off is
// width * height - the sum of the clipped bins: one pass over the 128 dwords gives both sums.
//
// stdif: mean and variance of the window from sum and sum of squares (unsigned int, as the reference's), then
// stdif.c:208-226 in double, step by step.
//
//   stdif_u8          a block of 256 threads makes 256 elements x `rows` rows (8; fewer where the tile of a tall window
//                     would not fit).  Pass 1: thread t takes staged columns t, t + 256 ..: the column's sum and sum of
//                     squares over the window's height for each of the block's rows (slide down: one row out, one in)
//                     into two LDS planes.  Pass 2: thread t adds `width` column sums for its element, then the
//                     doubles.  Integer sums do not depend on their order; the doubles are made with __dmul_rn /
//                     __dadd_rn / __ddiv_rn and sqrt(): no fused multiply-add, correctly rounded / and sqrt.
//                     The store: res < 0 -> 0, res >= 256 -> 255, else (unsigned char) (res + 0.5) -- and for 255.5 <=
//                     res < 256 that is 256.x converted to a byte, which the x86 reference does with cvttsd2si and a
//                     byte move: 0.  The kernel does the same: v_cvt_i32_f64, low byte.  s0 + b * sig == 0 divides
//                     by zero: undefined here as there.
#include "nbhd_tile.h"

#include <cstdint>

namespace vh {

constexpr int HL_LDS_MAX = 160 * 1024; // a CU's LDS

constexpr int HL_THREADS = 128;
constexpr int HL_TH = 8;                     // rows a block makes
constexpr int HL_LPR = HL_THREADS / HL_TH;   // lanes that share a row: (16 / bands) runs x bands
constexpr int HL_RUN = 16;                   // pels a lane slides over
constexpr int HL_BIN_DWORDS = 128;           // 256 bins of 16 bits
constexpr int HL_BINS_BYTES = HL_THREADS * HL_BIN_DWORDS * 4;
constexpr int HL_MAX_SIDE = 256;
constexpr int HL_MAX_AREA = 65535;           // a bin is 16 bits

constexpr int HLC_THREADS = 256;
constexpr int HLC_TW = 256; // elements
constexpr int HLC_TH = 8;   // rows
constexpr int HLC_MAX_AREA = 64;

typedef unsigned short hl_us2 __attribute__((ext_vector_type(2)));
VH_DEV unsigned int hl_pk_min(unsigned int a, unsigned int b)
{
	return __builtin_bit_cast(unsigned int, __builtin_elementwise_min(__builtin_bit_cast(hl_us2, a), __builtin_bit_cast(hl_us2, b)));
}
VH_DEV unsigned int hl_halves(unsigned int both) { return (both & 0xffffu) + (both >> 16); }

// bins: the lane's dword 0; value v is half v & 1 of dword v >> 1
VH_DEV void hl_put(unsigned int *bins, unsigned int v) { atomicAdd(bins + (v >> 1) * HL_THREADS, (v & 1u) ? 0x10000u : 1u); }
VH_DEV void hl_take(unsigned int *bins, unsigned int v) { atomicAdd(bins + (v >> 1) * HL_THREADS, (v & 1u) ? 0xffff0000u : 0xffffffffu); }

VH_DEV void hl_store(const NbArgs &a, int y, int e, unsigned int v)
{
	gstore8(gptr_out_of((unsigned long long) a.out + (unsigned long long) y * (unsigned long long) a.out_stride + (unsigned long long) e),
		(unsigned char) v);
}

template <bool CLAHE>
__global__ void __launch_bounds__(HL_THREADS)
hist_local_slide_kernel(NbArgs a, int max_slope, int groups)
{
	VH_DYNAMIC_LDS(unsigned int, lds);

	const int pel0 = (int) blockIdx.x * groups * HL_RUN; // the tile's first pel, of the output rect's row
	const int y0 = (int) blockIdx.y * HL_TH;
	const int s = (a.out_left + pel0 - a.win_w / 2) * a.bands;
	const int s_al = s & ~3; // (rounds down for negative s too)
	const int lead = s - s_al;
	const int rows = HL_TH + a.win_h - 1;
	nb_stage<1, false, true>(a, lds, s_al, a.out_top + y0 - a.win_h / 2, rows, HL_THREADS);

	const int t = tid();
	unsigned int *bins = lds + ((rows * a.lds_row) >> 2) + t;
	for (int d = 0; d < HL_BIN_DWORDS; d++)
		bins[d * HL_THREADS] = 0;
	barrier();

	const int ty = t / HL_LPR, j = t - ty * HL_LPR;
	const int g = j / a.bands, b = j - g * a.bands;
	const int x0 = pel0 + g * HL_RUN;
	if (g >= groups || y0 + ty >= a.out_height || x0 >= a.out_width)
		return;
	const int run = a.out_width - x0 < HL_RUN ? a.out_width - x0 : HL_RUN;
	const int n = a.win_w * a.win_h;
	const int step = a.bands;
	// the window of the run's first pel: its top-left element, this lane's band
	const unsigned char *p = (const unsigned char *) lds + ty * a.lds_row + lead + g * HL_RUN * step + b;

	for (int r = 0; r < a.win_h; r++) {
		const unsigned char *row = p + r * a.lds_row;
		for (int i = 0; i < a.win_w; i++)
			hl_put(bins, row[i * step]);
	}
	const unsigned int slope2 = (unsigned int) max_slope * 0x10001u;
	const unsigned char *centre = p + (a.win_h / 2) * a.lds_row + (a.win_w / 2) * step;
	for (int k = 0; k < run; k++) {
		const unsigned int target = centre[k * step];
		const int td = (int) (target >> 1);
		unsigned int below = 0, sum;
		if constexpr (CLAHE) {
			// hist_local.c:211-238: sum of min(hist, max_slope) up to the target, + (target + 1) * clipped / 256
			unsigned int all = 0;
			for (int d = 0; d < td; d++)
				below += hl_pk_min(bins[d * HL_THREADS], slope2);
			const unsigned int last = hl_pk_min(bins[td * HL_THREADS], slope2);
			for (int d = td + 1; d < HL_BIN_DWORDS; d++)
				all += hl_pk_min(bins[d * HL_THREADS], slope2);
			const unsigned int upto = hl_halves(below) + (last & 0xffffu) + ((target & 1u) ? last >> 16 : 0u);
			const unsigned int clipped = (unsigned int) n - (hl_halves(below) + hl_halves(last) + hl_halves(all));
			sum = upto + (target + 1u) * clipped / 256u;
		}
		else {
			for (int d = 0; d < td; d++)
				below += bins[d * HL_THREADS];
			const unsigned int last = bins[td * HL_THREADS];
			sum = hl_halves(below) + (last & 0xffffu) + ((target & 1u) ? last >> 16 : 0u);
		}
		hl_store(a, y0 + ty, (x0 + k) * step + b, 255u * sum / (unsigned int) n);
		if (k + 1 < run) {
			const unsigned char *col = p + k * step;
			for (int r = 0; r < a.win_h; r++) {
				hl_take(bins, col[r * a.lds_row]);
				hl_put(bins, col[r * a.lds_row + a.win_w * step]);
			}
		}
	}
}

__global__ void __launch_bounds__(HLC_THREADS)
hist_local_count_kernel(NbArgs a)
{
	VH_DYNAMIC_LDS(unsigned int, lds);

	const int out_e0 = a.out_left * a.bands + (int) blockIdx.x * HLC_TW;
	const int y0 = (int) blockIdx.y * HLC_TH;
	const int s = out_e0 - (a.win_w / 2) * a.bands;
	const int s_al = s & ~3;
	const int lead = s - s_al;
	nb_stage<1, false, true>(a, lds, s_al, a.out_top + y0 - a.win_h / 2, HLC_TH + a.win_h - 1, HLC_THREADS);
	barrier();

	const int t = tid();
	const int e = (int) blockIdx.x * HLC_TW + t; // of the output rect's row
	if (e >= a.out_width * a.bands)
		return;
	const unsigned int n = (unsigned int) (a.win_w * a.win_h);
	const unsigned char *keys = (const unsigned char *) lds + lead + t;
	for (int ty = 0; ty < HLC_TH; ty++) {
		if (y0 + ty >= a.out_height)
			break;
		const unsigned int target = keys[(ty + a.win_h / 2) * a.lds_row + (a.win_w / 2) * a.bands];
		unsigned int sum = 0;
		for (int r = 0; r < a.win_h; r++) {
			const unsigned char *row = keys + (ty + r) * a.lds_row;
			for (int i = 0; i < a.win_w; i++)
				sum += row[i * a.bands] <= target ? 1u : 0u;
		}
		hl_store(a, y0 + ty, e, 255u * sum / n);
	}
}

// ---- stdif

constexpr int SD_THREADS = 256;
constexpr int SD_TW = 256; // elements
constexpr int SD_TH = 8;   // rows, at most
constexpr int SD_MAX_AREA = 66051; // 255^2 * 66051 < 2^32 <= 255^2 * 66052: above it the reference's sum2 wraps

__global__ void __launch_bounds__(SD_THREADS)
stdif_kernel(StdifArgs sa)
{
	VH_DYNAMIC_LDS(unsigned int, lds);
	const NbArgs &a = sa.nb;

	const int out_e0 = a.out_left * a.bands + (int) blockIdx.x * SD_TW;
	const int y0 = (int) blockIdx.y * sa.rows;
	const int s = out_e0 - (a.win_w / 2) * a.bands;
	const int s_al = s & ~3;
	const int lead = s - s_al;
	const int rows = sa.rows + a.win_h - 1;
	nb_stage<1, false>(a, lds, s_al, a.out_top + y0 - a.win_h / 2, rows, SD_THREADS);
	barrier();

	// pass 1: the column sums of every staged column the block's elements read, for each of its rows
	const int t = tid();
	const int cols = SD_TW + (a.win_w - 1) * a.bands;
	unsigned int *plane = lds + ((rows * a.lds_row) >> 2); // [row][0: sum, 1: sum of squares][col]
	const unsigned char *keys = (const unsigned char *) lds + lead;
	for (int c = t; c < cols; c += SD_THREADS) {
		const unsigned char *col = keys + c;
		unsigned int sum = 0, sum2 = 0;
		for (int r = 0; r < a.win_h; r++) {
			const unsigned int v = col[r * a.lds_row];
			sum += v;
			sum2 += v * v;
		}
		for (int ty = 0; ty < sa.rows; ty++) {
			plane[(2 * ty) * cols + c] = sum;
			plane[(2 * ty + 1) * cols + c] = sum2;
			if (ty + 1 < sa.rows) {
				const unsigned int v0 = col[ty * a.lds_row], v1 = col[(ty + a.win_h) * a.lds_row];
				sum += v1 - v0;
				sum2 += v1 * v1 - v0 * v0;
			}
		}
	}
	barrier();

	const int e = (int) blockIdx.x * SD_TW + t; // of the output rect's row
	if (e >= a.out_width * a.bands)
		return;
	const double npel = (double) (a.win_w * a.win_h);
	for (int ty = 0; ty < sa.rows; ty++) {
		if (y0 + ty >= a.out_height)
			break;
		const unsigned int *ps = plane + (2 * ty) * cols + t, *ps2 = ps + cols;
		unsigned int sum = 0, sum2 = 0;
		for (int i = 0; i < a.win_w; i++) {
			sum += ps[i * a.bands];
			sum2 += ps2[i * a.bands];
		}
		const unsigned int centre = keys[(ty + a.win_h / 2) * a.lds_row + t + (a.win_w / 2) * a.bands];
		// stdif.c:208-217
		const double mean = __ddiv_rn((double) sum, npel);
		const double var = __dsub_rn(__ddiv_rn((double) sum2, npel), __dmul_rn(mean, mean));
		const double sig = sqrt(var);
		const double gain = __ddiv_rn(sa.f3, __dadd_rn(sa.s0, __dmul_rn(sa.b, sig)));
		const double res = __dadd_rn(__dadd_rn(sa.f1, __dmul_rn(sa.f2, mean)), __dmul_rn(__dsub_rn((double) centre, mean), gain));
		// :221-226; the last arm through the converter and a byte move, as the reference's machine does it
		unsigned int v;
		if (res < 0.0)
			v = 0;
		else if (res >= 256.0)
			v = 255;
		else
			v = (unsigned int) cvt_i32(__dadd_rn(res, 0.5)) & 255u;
		hl_store(a, y0 + ty, e, v);
	}
}

// bytes of a staged row: the lead of the rounding, `elems` elements; whole 16-byte groups
static long long hl_lds_row(long long elems)
{
	return (3 + elems + 15) / 16 * 16;
}

template <typename K, typename... A>
static int hl_launch(K kernel, const char *gate_name, dim3 grid, int threads, size_t lds, A... args)
{
	if (lds > 64 * 1024)
		VH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, HL_LDS_MAX));
	Gate gate(gate_name);
	hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, stream(), args...);
	VH_CHECK(hipGetLastError());
	return 0;
}

// Everything about the regions has been checked (ops_histogram.cpp); the image is uchar.
int hist_local_run(const char *domain, NbArgs a, int max_slope)
{
	const long long n = (long long) a.win_w * a.win_h;
	if (max_slope == 0 && n <= HLC_MAX_AREA) {
		a.lds_row = (int) hl_lds_row(HLC_TW + (long long) (a.win_w - 1) * a.bands);
		const long long lds = (long long) (HLC_TH + a.win_h - 1) * a.lds_row;
		if (lds > HL_LDS_MAX) {
			error(domain, "a %d x %d window on %d-band images needs %lld KB of LDS, the kernel has %d", a.win_w, a.win_h, a.bands,
				(lds + 1023) / 1024, HL_LDS_MAX / 1024);
			return -1;
		}
		const long long out_elems = (long long) a.out_width * a.bands;
		const dim3 grid((unsigned int) ((out_elems + HLC_TW - 1) / HLC_TW), (unsigned int) ((a.out_height + HLC_TH - 1) / HLC_TH), 1);
		return hl_launch(hist_local_count_kernel, "hist_local_count", grid, HLC_THREADS, (size_t) lds, a);
	}
	if (n > HL_MAX_AREA || a.win_w > HL_MAX_SIDE || a.win_h > HL_MAX_SIDE) {
		error(domain, "a %d x %d window: the kernel's 16-bit bins take windows of up to %d pels, %d a side", a.win_w, a.win_h,
			HL_MAX_AREA, HL_MAX_SIDE);
		return -1;
	}
	if (a.bands > HL_LPR) {
		error(domain, "%d-band images: the kernel takes up to %d bands", a.bands, HL_LPR);
		return -1;
	}
	const int groups = HL_LPR / a.bands;
	a.lds_row = (int) hl_lds_row((long long) (groups * HL_RUN + a.win_w - 1) * a.bands);
	const long long lds = (long long) (HL_TH + a.win_h - 1) * a.lds_row + HL_BINS_BYTES;
	if (lds > HL_LDS_MAX) {
		error(domain, "a %d x %d window on %d-band images needs %lld KB of LDS, the kernel has %d", a.win_w, a.win_h, a.bands,
			(lds + 1023) / 1024, HL_LDS_MAX / 1024);
		return -1;
	}
	const int tile_pels = groups * HL_RUN;
	const dim3 grid((unsigned int) ((a.out_width + tile_pels - 1) / tile_pels), (unsigned int) ((a.out_height + HL_TH - 1) / HL_TH), 1);
	if (max_slope > 0)
		return hl_launch(hist_local_slide_kernel<true>, "hist_local_slide", grid, HL_THREADS, (size_t) lds, a, max_slope, groups);
	return hl_launch(hist_local_slide_kernel<false>, "hist_local_slide", grid, HL_THREADS, (size_t) lds, a, 0, groups);
}

int hist_local_tile(int what)
{
	switch (what) {
	case 0: return HL_RUN;
	case 1: return HL_TH;
	case 2: return HL_MAX_SIDE;
	case 3: return HL_LPR;
	case 4: return HLC_MAX_AREA;
	case 5: return HLC_TW;
	case 6: return HLC_TH;
	default: return 0;
	}
}

int stdif_run(const char *domain, StdifArgs sa)
{
	NbArgs &a = sa.nb;
	const long long n = (long long) a.win_w * a.win_h;
	if (n > SD_MAX_AREA) {
		error(domain, "a %d x %d window has %lld pels: above %d the sum of squares leaves 32 bits", a.win_w, a.win_h, n, SD_MAX_AREA);
		return -1;
	}
	const long long cols = SD_TW + (long long) (a.win_w - 1) * a.bands;
	a.lds_row = (int) hl_lds_row(cols);
	long long lds = 0;
	for (sa.rows = SD_TH; sa.rows >= 1; sa.rows /= 2) {
		lds = (long long) (sa.rows + a.win_h - 1) * a.lds_row + 2LL * sa.rows * cols * 4;
		if (lds <= HL_LDS_MAX)
			break;
	}
	if (sa.rows < 1) {
		error(domain, "a %d x %d window on %d-band images needs %lld KB of LDS, the kernel has %d", a.win_w, a.win_h, a.bands,
			(lds + 1023) / 1024, HL_LDS_MAX / 1024);
		return -1;
	}
	const long long out_elems = (long long) a.out_width * a.bands;
	const dim3 grid((unsigned int) ((out_elems + SD_TW - 1) / SD_TW), (unsigned int) ((a.out_height + sa.rows - 1) / sa.rows), 1);
	if (grid.y > 65535) { // (rows of blocks go in the grid's y)
		error(domain, "image too large");
		return -1;
	}
	return hl_launch(stdif_kernel, "stdif_u8", grid, SD_THREADS, (size_t) lds, sa);
}

int stdif_tile(int what)
{
	return what == 0 ? SD_TW : what == 1 ? SD_TH : what == 2 ? SD_MAX_AREA : 0;
}

} // namespace vh
