// vips_labelregions and vips_countlines (morphology/labelregions.c, countlines.c) on the device (gfx950).
//
// labelregions: the regions are the 4-connected components of pels that are bytewise equal over the whole pel
// (draw_flood.c:223-235), numbered from 1 in raster order of each region's first pel (labelregions.c:86-102).  The
// raster-first pel of a region is the pel with the smallest linear index y * width + x, so a union-find whose links always
// point to the SMALLER index ends with every region's root at the pel the reference floods from, whatever order the
// atomics land in; numbering the roots in index order is then the reference's numbering.  Six launches; the launch
// boundary is the only synchronisation between them, and no loop waits for another thread: every loop ends because an
// index strictly decreases (a link only ever points down) or strictly advances.
//
//   label_tiles<UNIT, ND>  a block owns a tile of REGIONS_TW x REGIONS_TH pels, a wave a row at a time (four rows, one
//                          below the other, so that the pel above is the wave's own previous row in registers).  A pel is
//                          read once as whole pels of up to ND dwords (in UNIT-byte loads: the largest of 4, 2, 1 that the
//                          pel size and the row starts are multiples of); the pels left of a tile and above a wave's first
//                          row are read a second time.  The read is reduced to two bits, "equal to my left neighbour" and
//                          "equal to the pel above"; nothing after that depends on the pel size.  Runs: the wave's ballot
//                          of the left bit, a run's first lane the highest clear bit at or below the lane.  Vertical
//                          unions between the runs of adjacent rows: a union-find on tile-local indices in LDS, atomicMin
//                          towards the smaller index, only where one of the two rows starts a run (every other pair is
//                          implied by its left neighbour's).  Every pel then writes the GLOBAL linear index of its
//                          tile-local root to the parent plane.
//                          The bits across the tile borders are KEPT, one byte a seam pel (vseam: the left bit of the
//                          first column of every tile column but the first; hseam: the up bit of the first row of every
//                          tile row but the first), and not recomputed by label_seams: that kernel then is one kernel for
//                          every pel size and reads no pel, at the price of (width / TW) * height + (height / TH) * width
//                          bytes written and read: 5 / 256 of one pass over a plane.
//   label_seams            a lane per seam byte; where it is set, the union of the two pels in the parent plane in global
//                          memory: find both roots, atomic min of the smaller into the larger root's slot, and on from the
//                          value the atomic returned when somebody else got there first.  EVERY access to the parent plane
//                          in this kernel is an agent-scope atomic (a relaxed agent-scope load, an agent-scope min): the
//                          blocks of one launch run on eight XCDs whose L2s do not see one another's plain stores, and a
//                          CU's L1 is never refreshed by another CU's, so a plain load here could return a parent that is
//                          no longer there.  (An old parent is still an ancestor, so the loop would survive it; the kernel
//                          does not lean on that.)
//   label_roots            plain loads from here on: the launch boundary made everything visible and nothing writes the
//                          plane being walked.  Every pel walks to its root and writes it to the OUTPUT plane; every chunk
//                          of REGIONS_CHUNK linear indices counts its roots (root == own index: ballot and popcount, one
//                          store a chunk).
//   label_scan             ONE block: the exclusive prefix sum of the chunk counts, in place, and the total.
//   label_serials          every root writes 1 + its chunk's offset + its rank inside the chunk (a ballot prefix) into the
//                          parent plane at its own index; the plane is free by now.
//   label_number           out[p] = parent[out[p]].
//
// countlines<T>: the reference's chain (moreeq_const 128, conv with (-1, 1) clipped to uchar, project, avg, / 255) counts
// RISES: an element below 128 followed -- down its column for `horizontal`, along its row for `vertical` -- by one at or
// above 128.  One read-only launch: the comparison is logic_elem's (logic_device.h), the rises of a wave are a ballot and
// a popcount, a block sends ONE 64-bit integer atomic add.
#include "logic_device.h"
#include "pointwise.h"

namespace vh {

constexpr int REGIONS_THREADS = 256;
constexpr int REGIONS_WAVES = REGIONS_THREADS / 64;
constexpr int REGIONS_TW = 64;                                // pels of a tile's row: a wave
constexpr int REGIONS_TH = 16;                                // rows of a tile
constexpr int REGIONS_WAVE_ROWS = REGIONS_TH / REGIONS_WAVES; // consecutive rows a wave owns
constexpr int REGIONS_CHUNK = 1024;                           // linear indices whose roots are counted together
constexpr int REGIONS_CHUNK_STEPS = REGIONS_CHUNK / REGIONS_THREADS;
constexpr int REGIONS_SCAN_THREADS = 1024;
constexpr int REGIONS_SCAN_WAVES = REGIONS_SCAN_THREADS / 64;
constexpr int REGIONS_SCAN_EACH = 4;                          // consecutive counts a lane of label_scan owns
constexpr int COUNTLINES_ROWS = 64;                           // rows of a block's strip
constexpr int COUNTLINES_GRID_BLOCKS = 2048;

static_assert(REGIONS_TW == 64, "a row of a tile is a wave");
static_assert(REGIONS_MAX_PEL == CANVAS_MAX_PEL && REGIONS_MAX_PEL == 32, "a pel is at most eight dwords");

struct RegionsArgs {
	const unsigned char *in;
	long long stride; // bytes
	int width, height;
	int pel;     // bytes
	int units;   // of UNIT bytes a pel
	int n;       // width * height
	int tiles_x; // tiles of a row of tiles
	int chunks;
	long long n_vseam, n_hseam;
	int *parent;           // n
	unsigned char *vseam;  // (tiles_x - 1) * height: [k * height + y] the left bit of pel ((k + 1) TW, y)
	unsigned char *hseam;  // (tiles_y - 1) * width: [k * width + x] the up bit of pel (x, (k + 1) TH)
	int *counts;           // chunks
	int *total;
	int *out;              // n: the mask
};

// ---------------------------------------------------------------- label_tiles

// the pel at p as ND dwords, zero behind its last byte
template <int UNIT, int ND>
VH_DEV void regions_pel(const unsigned char *p, int units, u32 (&d)[ND])
{
#pragma unroll
	for (int i = 0; i < ND; i++)
		d[i] = 0;
	if constexpr (UNIT == 4) {
#pragma unroll
		for (int i = 0; i < ND; i++)
			if (i < units)
				d[i] = ((const u32 *) p)[i];
	}
	else if constexpr (UNIT == 2) {
#pragma unroll
		for (int i = 0; i < 2 * ND; i++)
			if (i < units)
				d[i >> 1] |= (u32) ((const u16 *) p)[i] << (16 * (i & 1));
	}
	else {
#pragma unroll
		for (int i = 0; i < 4 * ND; i++)
			if (i < units)
				d[i >> 2] |= (u32) p[i] << (8 * (i & 3));
	}
}

// the root of tile-local index i: a link only points down, so i strictly decreases.  (volatile: other lanes link
// while this one walks)
VH_DEV int regions_lds_find(int *lab, int i)
{
	for (;;) {
		const int p = ((volatile int *) lab)[i];
		if (p >= i) // (p == i: a root; a slot never holds more than its own index)
			return i;
		i = p;
	}
}

VH_DEV void regions_lds_union(int *lab, int a, int b)
{
	for (;;) {
		a = regions_lds_find(lab, a);
		b = regions_lds_find(lab, b);
		if (a == b)
			return;
		if (a < b) {
			const int t = a;
			a = b;
			b = t;
		}
		// a is the larger root: its slot takes the smaller.  Somebody else linked it first: the slot held old < a, the
		// union to make is now that of old and b
		const int old = atomicMin(lab + a, b);
		if (old >= a)
			return;
		a = old;
	}
}

template <int UNIT, int ND>
__global__ void __launch_bounds__(REGIONS_THREADS)
label_tiles_kernel(RegionsArgs a)
{
	__shared__ int s_lab[REGIONS_TW * REGIONS_TH];
	__shared__ u64 s_left[REGIONS_TH]; // every row's ballot of the left bit inside the tile

	const int t = tid();
	const int lane = t & 63, wave = t >> 6;
	// (the tiles as one sequence: a tall image has more rows of tiles than a grid has in y)
	const int tile_y = (int) (blockIdx.x / (u32) a.tiles_x), tile_x = (int) (blockIdx.x - (u32) tile_y * (u32) a.tiles_x);
	const int tx0 = tile_x * REGIONS_TW, ty0 = tile_y * REGIONS_TH;
	const int x = tx0 + lane;
	const bool in_x = x < a.width;
	const unsigned char *column = a.in + (long long) x * a.pel;

	u32 above[ND];
	bool joins[REGIONS_WAVE_ROWS]; // the pel equals the one above, and that one lies in this tile
#pragma unroll
	for (int k = 0; k < REGIONS_WAVE_ROWS; k++) {
		const int r = wave * REGIONS_WAVE_ROWS + k;
		const int y = ty0 + r;
		const bool inside = in_x && y < a.height;
		u32 cur[ND], left_pel[ND];
#pragma unroll
		for (int i = 0; i < ND; i++)
			cur[i] = 0;
		if (inside)
			regions_pel<UNIT, ND>(column + (long long) y * a.stride, a.units, cur);
		if (k == 0) {
			// the row above the wave's first: another wave's, or another tile's
#pragma unroll
			for (int i = 0; i < ND; i++)
				above[i] = 0;
			if (inside && y > 0)
				regions_pel<UNIT, ND>(column + (long long) (y - 1) * a.stride, a.units, above);
		}
#pragma unroll
		for (int i = 0; i < ND; i++)
			left_pel[i] = lane_prev(cur[i]);
		if (lane == 0) {
			// the pel left of the tile
#pragma unroll
			for (int i = 0; i < ND; i++)
				left_pel[i] = 0;
			if (inside && x > 0)
				regions_pel<UNIT, ND>(column + (long long) y * a.stride - a.pel, a.units, left_pel);
		}
		bool up = inside && y > 0, left = inside && x > 0;
#pragma unroll
		for (int i = 0; i < ND; i++) {
			up = up && cur[i] == above[i];
			left = left && cur[i] == left_pel[i];
			above[i] = cur[i];
		}
		// the seams' bits, for label_seams
		if (lane == 0 && tile_x > 0 && inside)
			a.vseam[(size_t) (tile_x - 1) * (size_t) a.height + (size_t) y] = left ? 1 : 0;
		if (r == 0 && tile_y > 0 && inside)
			a.hseam[(size_t) (tile_y - 1) * (size_t) a.width + (size_t) x] = up ? 1 : 0;
		// the runs of the row: a run's first lane is the highest clear bit at or below the lane (bit 0 is always clear)
		const u64 bits = __builtin_amdgcn_ballot_w64(left && lane > 0);
		const u64 clear = ~bits & (~0ull >> (63 - lane));
		const int first = 63 - __builtin_clzll(clear);
		s_lab[r * REGIONS_TW + lane] = r * REGIONS_TW + first;
		if (lane == 0)
			s_left[r] = bits;
		joins[k] = up && r > 0;
	}
	barrier();
	// the runs of adjacent rows: where both rows go on from their left neighbours, that neighbour's pair says the same
#pragma unroll
	for (int k = 0; k < REGIONS_WAVE_ROWS; k++) {
		const int r = wave * REGIONS_WAVE_ROWS + k;
		if (joins[k] && !(((s_left[r] & s_left[r - 1]) >> lane) & 1))
			regions_lds_union(s_lab, r * REGIONS_TW + lane, (r - 1) * REGIONS_TW + lane);
	}
	barrier();
#pragma unroll
	for (int k = 0; k < REGIONS_WAVE_ROWS; k++) {
		const int r = wave * REGIONS_WAVE_ROWS + k;
		const int y = ty0 + r;
		if (in_x && y < a.height) {
			// (the tile's indices and the image's are both in raster order: the tile's smallest is the image's smallest)
			const int root = regions_lds_find(s_lab, r * REGIONS_TW + lane);
			const int ry = root / REGIONS_TW, rx = root - ry * REGIONS_TW;
			a.parent[(size_t) y * (size_t) a.width + (size_t) x] = (ty0 + ry) * a.width + tx0 + rx;
		}
	}
}

// ---------------------------------------------------------------- label_seams

#define REGIONS_LOAD_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define REGIONS_MIN_AGENT(p, v) __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

VH_DEV int regions_find_agent(int *parent, int i)
{
	for (;;) {
		const int p = REGIONS_LOAD_AGENT(parent + i);
		if (p >= i)
			return i;
		i = p;
	}
}

VH_DEV void regions_union_agent(int *parent, int a, int b)
{
	for (;;) {
		a = regions_find_agent(parent, a);
		b = regions_find_agent(parent, b);
		if (a == b)
			return;
		if (a < b) {
			const int t = a;
			a = b;
			b = t;
		}
		const int old = REGIONS_MIN_AGENT(parent + a, b);
		if (old >= a)
			return;
		a = old; // somebody linked a first, to old < a: old and b are to be joined now
	}
}

__global__ void __launch_bounds__(REGIONS_THREADS)
label_seams_kernel(RegionsArgs a)
{
	const long long at = (long long) blockIdx.x * REGIONS_THREADS + tid();
	if (at < a.n_vseam) {
		// the left bit of pel ((k + 1) TW, y)
		if (!a.vseam[at])
			return;
		const int k = (int) (at / a.height), y = (int) (at - (long long) k * a.height);
		const int p = y * a.width + (k + 1) * REGIONS_TW;
		regions_union_agent(a.parent, p, p - 1);
	}
	else if (at < a.n_vseam + a.n_hseam) {
		// the up bit of pel (x, (k + 1) TH)
		const long long j = at - a.n_vseam;
		if (!a.hseam[j])
			return;
		const int k = (int) (j / a.width), x = (int) (j - (long long) k * a.width);
		const int p = (k + 1) * REGIONS_TH * a.width + x;
		regions_union_agent(a.parent, p, p - a.width);
	}
}

// ---------------------------------------------------------------- label_roots, label_scan, label_serials, label_number

__global__ void __launch_bounds__(REGIONS_THREADS)
label_roots_kernel(RegionsArgs a)
{
	__shared__ int s_count[REGIONS_WAVES];
	const int t = tid();
	int count = 0;
#pragma unroll
	for (int k = 0; k < REGIONS_CHUNK_STEPS; k++) {
		const u32 i = (u32) blockIdx.x * REGIONS_CHUNK + (u32) (k * REGIONS_THREADS + t);
		const bool inside = i < (u32) a.n;
		int root = -1;
		if (inside) {
			root = (int) i;
			for (;;) {
				const int p = a.parent[root];
				if (p >= root)
					break;
				root = p;
			}
			a.out[i] = root;
		}
		count += __builtin_popcountll(__builtin_amdgcn_ballot_w64(inside && root == (int) i));
	}
	if ((t & 63) == 0)
		s_count[t >> 6] = count;
	barrier();
	if (t == 0) {
		int sum = 0;
#pragma unroll
		for (int w = 0; w < REGIONS_WAVES; w++)
			sum += s_count[w];
		a.counts[blockIdx.x] = sum;
	}
}

// counts[i] becomes the sum of the counts before it; *total the sum of all of them.  One block; the loop advances by
// REGIONS_SCAN_THREADS * REGIONS_SCAN_EACH counts a turn.
__global__ void __launch_bounds__(REGIONS_SCAN_THREADS)
label_scan_kernel(RegionsArgs a)
{
	__shared__ int s_wave[REGIONS_SCAN_WAVES];
	const int t = tid();
	const int lane = t & 63, wave = t >> 6;
	int carry = 0;
	for (int base = 0; base < a.chunks; base += REGIONS_SCAN_THREADS * REGIONS_SCAN_EACH) {
		const int i0 = base + t * REGIONS_SCAN_EACH;
		int v[REGIONS_SCAN_EACH], mine = 0;
#pragma unroll
		for (int j = 0; j < REGIONS_SCAN_EACH; j++) {
			v[j] = i0 + j < a.chunks ? a.counts[i0 + j] : 0;
			mine += v[j];
		}
		// the wave's inclusive sums
		int sum = mine;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const int o = (int) lane_from((u32) sum, -d);
			sum += lane >= d ? o : 0;
		}
		if (lane == 63)
			s_wave[wave] = sum;
		barrier();
		int before = carry, all = 0;
#pragma unroll
		for (int w = 0; w < REGIONS_SCAN_WAVES; w++) {
			const int s = s_wave[w];
			before += w < wave ? s : 0;
			all += s;
		}
		int at = before + sum - mine;
#pragma unroll
		for (int j = 0; j < REGIONS_SCAN_EACH; j++) {
			if (i0 + j < a.chunks)
				a.counts[i0 + j] = at;
			at += v[j];
		}
		carry += all;
		barrier(); // (s_wave is written again next turn)
	}
	if (t == 0)
		*a.total = carry;
}

__global__ void __launch_bounds__(REGIONS_THREADS)
label_serials_kernel(RegionsArgs a)
{
	__shared__ int s_count[REGIONS_CHUNK_STEPS * REGIONS_WAVES];
	const int t = tid();
	const int lane = t & 63, wave = t >> 6;
	bool is_root[REGIONS_CHUNK_STEPS];
	int rank[REGIONS_CHUNK_STEPS];
#pragma unroll
	for (int k = 0; k < REGIONS_CHUNK_STEPS; k++) {
		const u32 i = (u32) blockIdx.x * REGIONS_CHUNK + (u32) (k * REGIONS_THREADS + t);
		is_root[k] = i < (u32) a.n && a.out[i] == (int) i;
		const u64 bits = __builtin_amdgcn_ballot_w64(is_root[k]);
		rank[k] = __builtin_popcountll(bits & ~(~0ull << lane)); // the roots of the wave before this lane
		if (lane == 0)
			s_count[k * REGIONS_WAVES + wave] = __builtin_popcountll(bits);
	}
	barrier();
	const int offset = a.counts[blockIdx.x];
#pragma unroll
	for (int k = 0; k < REGIONS_CHUNK_STEPS; k++) {
		// the chunk's indices run over the steps, then the waves, then the lanes
		int before = 0;
#pragma unroll
		for (int j = 0; j < REGIONS_CHUNK_STEPS * REGIONS_WAVES; j++)
			before += j < k * REGIONS_WAVES + wave ? s_count[j] : 0;
		if (is_root[k]) {
			const u32 i = (u32) blockIdx.x * REGIONS_CHUNK + (u32) (k * REGIONS_THREADS + t);
			a.parent[i] = 1 + offset + before + rank[k];
		}
	}
}

__global__ void __launch_bounds__(REGIONS_THREADS)
label_number_kernel(RegionsArgs a)
{
#pragma unroll
	for (int k = 0; k < REGIONS_CHUNK_STEPS; k++) {
		const u32 i = (u32) blockIdx.x * REGIONS_CHUNK + (u32) (k * REGIONS_THREADS + tid());
		if (i < (u32) a.n)
			a.out[i] = a.parent[a.out[i]];
	}
}

// ---------------------------------------------------------------- countlines

struct CountlinesArgs {
	const unsigned char *in;
	u64 *rises;       // zero before the launch
	long long stride; // bytes
	int elems;        // width * bands
	int height, bands;
	int vertical;     // along the rows
};

// vips_moreeq_const1(in, 128): an integer format compares integers, relational.c:528-529
template <typename T>
VH_DEV bool countlines_white(T v)
{
	return logic_elem<LOGIC_RELATIONAL, RELATIONAL_MOREEQ, true, T>(v, (T) 0, !std::is_floating_point<T>::value, 128, 128.0) != 0;
}

template <typename T>
__global__ void __launch_bounds__(REGIONS_THREADS)
countlines_kernel(CountlinesArgs a)
{
	__shared__ u64 s_count[REGIONS_WAVES];
	const int t = tid();
	const long long el = (long long) blockIdx.x * REGIONS_THREADS + t;
	const bool in_x = el < a.elems;
	const size_t e = in_x ? (size_t) el : 0;
	u64 count = 0;
	for (int y0 = (int) blockIdx.y * COUNTLINES_ROWS; y0 < a.height; y0 += (int) gridDim.y * COUNTLINES_ROWS) {
		const int rows = min(COUNTLINES_ROWS, a.height - y0);
		// horizontal: the element above; the copied edge above row 0 makes no transition
		bool before = true;
		if (!a.vertical && in_x && y0 > 0)
			before = countlines_white<T>(((const T *) (a.in + (long long) (y0 - 1) * a.stride))[e]);
		for (int r = 0; r < rows; r++) {
			const T *row = (const T *) (a.in + (long long) (y0 + r) * a.stride);
			bool white = true;
			if (in_x)
				white = countlines_white<T>(row[e]);
			if (a.vertical) {
				// the same band of the pel to the left; the copied edge left of column 0 makes no transition
				before = true;
				if (in_x && e >= (size_t) a.bands)
					before = countlines_white<T>(row[e - a.bands]);
			}
			count += (u64) __builtin_popcountll(__builtin_amdgcn_ballot_w64(in_x && white && !before));
			before = white;
		}
	}
	if ((t & 63) == 0)
		s_count[t >> 6] = count;
	barrier();
	if (t == 0) {
		u64 sum = 0;
#pragma unroll
		for (int w = 0; w < REGIONS_WAVES; w++)
			sum += s_count[w];
		if (sum)
			atomicAdd((unsigned long long *) a.rises, (unsigned long long) sum);
	}
}

// ---------------------------------------------------------------- launches

template <int UNIT>
static void label_tiles_launch(int nd, dim3 grid, const RegionsArgs &a)
{
	const dim3 block(REGIONS_THREADS, 1, 1);
	switch (nd) {
	case 1: hipLaunchKernelGGL((label_tiles_kernel<UNIT, 1>), grid, block, 0, stream(), a); break;
	case 2: hipLaunchKernelGGL((label_tiles_kernel<UNIT, 2>), grid, block, 0, stream(), a); break;
	case 4: hipLaunchKernelGGL((label_tiles_kernel<UNIT, 4>), grid, block, 0, stream(), a); break;
	default: hipLaunchKernelGGL((label_tiles_kernel<UNIT, 8>), grid, block, 0, stream(), a); break;
	}
}

void regions_layout(int width, int height, RegionsLayout *l)
{
	const size_t n = (size_t) width * (size_t) height;
	const size_t tiles_x = ((size_t) width + REGIONS_TW - 1) / REGIONS_TW, tiles_y = ((size_t) height + REGIONS_TH - 1) / REGIONS_TH;
	auto round = [](size_t v) { return (v + 255) / 256 * 256; };
	l->chunks = (int) ((n + REGIONS_CHUNK - 1) / REGIONS_CHUNK);
	l->n_vseam = (long long) ((tiles_x - 1) * (size_t) height);
	l->n_hseam = (long long) ((tiles_y - 1) * (size_t) width);
	l->parent = 0;
	l->vseam = round(n * sizeof(int));
	l->hseam = l->vseam + round((size_t) l->n_vseam);
	l->counts = l->hseam + round((size_t) l->n_hseam);
	l->total = l->counts + round((size_t) l->chunks * sizeof(int));
	l->bytes = l->total + 256;
}

// Everything has been checked (ops_regions.cpp): a real format, a pel of at most REGIONS_MAX_PEL bytes, fewer than 2^31
// pels, rows that start on whole elements.  `planes` holds regions_layout()'s bytes, `out` width * height ints; every
// byte of both that is read is written first.  The total lands in the int at planes + layout.total.
int regions_label_run(const char *domain, const _VipsHipImage *in, unsigned char *planes, int *out)
{
	RegionsLayout l;
	regions_layout(in->width, in->height, &l);
	RegionsArgs a = {};
	a.in = (const unsigned char *) in->data;
	a.stride = (long long) in->stride;
	a.width = in->width;
	a.height = in->height;
	a.pel = in->bands * format_sizeof(in->format);
	a.n = in->width * in->height;
	a.parent = (int *) (planes + l.parent);
	a.vseam = planes + l.vseam;
	a.hseam = planes + l.hseam;
	a.counts = (int *) (planes + l.counts);
	a.total = (int *) (planes + l.total);
	a.out = out;
	a.chunks = l.chunks;
	a.n_vseam = l.n_vseam;
	a.n_hseam = l.n_hseam;
	const uintptr_t starts = (uintptr_t) in->data | (uintptr_t) in->stride | (uintptr_t) a.pel;
	const int unit = starts % 4 == 0 ? 4 : starts % 2 == 0 ? 2 : 1;
	a.units = a.pel / unit;
	const int nd = a.pel <= 4 ? 1 : a.pel <= 8 ? 2 : a.pel <= 16 ? 4 : 8;
	const unsigned int tiles_x = (unsigned int) ((in->width + REGIONS_TW - 1) / REGIONS_TW);
	const unsigned int tiles_y = (unsigned int) ((in->height + REGIONS_TH - 1) / REGIONS_TH);
	a.tiles_x = (int) tiles_x;
	if (a.pel < 1 || a.pel > REGIONS_MAX_PEL || (long long) in->width * in->height >= (1LL << 31)) {
		error(domain, "image outside the kernels' range");
		return -1;
	}
	const dim3 block(REGIONS_THREADS, 1, 1), chunks((unsigned int) l.chunks, 1, 1);
	{
		Gate gate("label_tiles");
		const dim3 grid(tiles_x * tiles_y, 1, 1); // (fewer than 2^31 / TH)
		switch (unit) {
		case 4: label_tiles_launch<4>(nd, grid, a); break;
		case 2: label_tiles_launch<2>(nd, grid, a); break;
		default: label_tiles_launch<1>(nd, grid, a); break;
		}
		VH_CHECK(hipGetLastError());
	}
	if (l.n_vseam + l.n_hseam > 0) {
		Gate gate("label_seams");
		const dim3 grid((unsigned int) ((l.n_vseam + l.n_hseam + REGIONS_THREADS - 1) / REGIONS_THREADS), 1, 1);
		hipLaunchKernelGGL(label_seams_kernel, grid, block, 0, stream(), a);
		VH_CHECK(hipGetLastError());
	}
	{
		Gate gate("label_roots");
		hipLaunchKernelGGL(label_roots_kernel, chunks, block, 0, stream(), a);
		VH_CHECK(hipGetLastError());
	}
	{
		Gate gate("label_scan");
		hipLaunchKernelGGL(label_scan_kernel, dim3(1, 1, 1), dim3(REGIONS_SCAN_THREADS, 1, 1), 0, stream(), a);
		VH_CHECK(hipGetLastError());
	}
	{
		Gate gate("label_serials");
		hipLaunchKernelGGL(label_serials_kernel, chunks, block, 0, stream(), a);
		VH_CHECK(hipGetLastError());
	}
	{
		Gate gate("label_number");
		hipLaunchKernelGGL(label_number_kernel, chunks, block, 0, stream(), a);
		VH_CHECK(hipGetLastError());
	}
	return 0;
}

template <typename T>
static int countlines_launch(const CountlinesArgs &a)
{
	const long long bx = ((long long) a.elems + REGIONS_THREADS - 1) / REGIONS_THREADS;
	long long by = (a.height + COUNTLINES_ROWS - 1) / COUNTLINES_ROWS;
	const long long cap = bx >= COUNTLINES_GRID_BLOCKS ? 1 : COUNTLINES_GRID_BLOCKS / bx;
	by = by > cap ? cap : by;
	Gate gate("countlines");
	hipLaunchKernelGGL((countlines_kernel<T>), dim3((unsigned int) bx, (unsigned int) by, 1), dim3(REGIONS_THREADS, 1, 1), 0, stream(), a);
	VH_CHECK(hipGetLastError());
	return 0;
}

// a real format, rows that start on whole elements, width * bands < 2^31; *rises (device memory) is zero
int countlines_run(const char *domain, const _VipsHipImage *in, int vertical, unsigned long long *rises)
{
	CountlinesArgs a = {};
	a.in = (const unsigned char *) in->data;
	a.rises = (u64 *) rises;
	a.stride = (long long) in->stride;
	a.elems = in->width * in->bands;
	a.height = in->height;
	a.bands = in->bands;
	a.vertical = vertical;
	switch (in->format) {
	case VIPS_HIP_FORMAT_UCHAR: return countlines_launch<u8>(a);
	case VIPS_HIP_FORMAT_CHAR: return countlines_launch<s8>(a);
	case VIPS_HIP_FORMAT_USHORT: return countlines_launch<u16>(a);
	case VIPS_HIP_FORMAT_SHORT: return countlines_launch<s16>(a);
	case VIPS_HIP_FORMAT_UINT: return countlines_launch<u32>(a);
	case VIPS_HIP_FORMAT_INT: return countlines_launch<s32>(a);
	case VIPS_HIP_FORMAT_FLOAT: return countlines_launch<f32>(a);
	case VIPS_HIP_FORMAT_DOUBLE: return countlines_launch<f64>(a);
	default:
		error(domain, "no kernel for format %d", in->format);
		return -1;
	}
}

int regions_tile(int what)
{
	switch (what) {
	case 0: return REGIONS_TW;
	case 1: return REGIONS_TH;
	case 2: return REGIONS_MAX_PEL;
	case 3: return REGIONS_CHUNK;
	default: return 0;
	}
}

} // namespace vh

extern "C" int vips_hip_countlines_step(int what)
{
	switch (what) {
	case 0: return vh::REGIONS_THREADS;
	case 1: return vh::COUNTLINES_ROWS;
	case 2: return vh::COUNTLINES_GRID_BLOCKS;
	default: return 0;
	}
}
