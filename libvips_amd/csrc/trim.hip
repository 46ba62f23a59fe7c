// vips_project, vips_profile (arithmetic/project.c, profile.c) and the fused scan of vips_find_trim (find_trim.c) on the
// device (gfx950).  All are read-only passes: nothing the size of the image is written.
//
//   project_stream<T, B>   B = 1 .. 4 bands, rows that start on dwords.  A lane owns ONE 16-byte group of a row -- 16 /
//                          sizeof(T) elements -- and walks down the rows of its block.  A column sum is a sum per ELEMENT
//                          of the row, so it is one register per element the lane owns and the band count plays no part.
//                          A row sum is per band: the lane adds its elements by (position mod B) relative to its first
//                          element (constant register indices), turns that into bands by selects, the wave adds its 64
//                          lanes by rotation (ds_bpermute), the four waves of a block meet in LDS once per tile of
//                          TRIM_ROWS rows.  Then ONE add per block and output element: an integer atomic for the integer
//                          formats (sums wrap mod 2^32 like the reference's guint / int accumulators), a partial for
//                          double sums.
//   project_general<T>     any band count and any row start: block (x, rows, band), one element a lane and row.
//   double sums            no floating atomics: block (bx, by, bz) writes its column partials to slab row `by` and its
//                          row partials to slab row `bx`; the block that takes the last ticket adds the slabs in index
//                          order and writes both outputs.  The order depends on the image's geometry alone, so the same
//                          image gives the same bits on every run.
//   profile<T>             the geometry of project_general.  A lane keeps the first y at which its element was non-zero
//                          (C's `if (p[j])`: a NaN counts, -0.0 does not); the x of a row's first non-zero element is a
//                          minimum over the wave, then over the block's waves in LDS; one integer atomic min per block
//                          and output element that has something to say.  The host fills the outputs with `height` /
//                          `width` first.
//   trim_fused<MEDIAN>     uchar, 1 .. 4 bands: rank.hip's packed 3 x 3 median network on the halo tile of nbhd_tile.h
//                          (the edges copy, as vips_rank's embed does), the median byte of every element looked up in a
//                          256 x bands predicate table (LDS), and the smallest and largest x and y of an element whose
//                          predicate holds -- the OR across the bands is implied: a pel is set when any of its elements
//                          is.  The bounds are kept as "larger is better" numbers (width - x, x + 1, height - y, y + 1;
//                          0: none), reduced over the wave and the block; a block reads the four results so far past
//                          the caches and only sends an atomic max for those it improves.  !MEDIAN (line_art) looks
//                          the centre byte up.
#include "nbhd_tile.h"
#include "pointwise.h"

namespace vh {

constexpr int TRIM_THREADS = 256;
constexpr int TRIM_WAVES = TRIM_THREADS / 64;
constexpr int TRIM_GROUP = 16;        // bytes of a row a lane of project_stream owns
constexpr int TRIM_ROWS = 16;         // rows between two meetings of a block's waves
constexpr int TRIM_AHEAD = 4;         // rows whose loads a lane of project_stream has in flight
constexpr int TRIM_GRID_BLOCKS = 1024; // of a launch, four a CU as stats (the grid's x is never capped: a lane owns its columns)
constexpr int TRIM_FUSED_TW = 256;    // elements of a fused tile's row
constexpr int TRIM_FUSED_TH = 8;      // rows of a fused tile
constexpr int TRIM_FUSED_TILES = 8;   // tiles, one below the other, of a fused block

struct ProjectArgs {
	const unsigned char *in;
	void *columns, *rows;       // the outputs: elems, height * bands sums
	f64 *col_part, *row_part;   // double sums: grid.y rows of elems, grid.x rows of height * bands partials
	u32 *ticket;                // double sums: zero before the launch
	long long stride;           // bytes
	int width, height, bands;
	int elems;                  // width * bands
};

// project.c:99-102 as accumulators: the integer formats add in 32 bits (int wraps as unsigned does here), float and
// double add doubles
template <typename T>
struct ProjectSum {
	typedef typename std::conditional<std::is_floating_point<T>::value, f64, u32>::type type;
};

template <typename T>
VH_DEV typename ProjectSum<T>::type project_value(T v)
{
	typedef typename ProjectSum<T>::type S;
	if constexpr (std::is_floating_point<T>::value)
		return (S) v;
	else
		return (S) (s32) v; // (sign-extended: the int the reference adds)
}

// what lane + delta of the wave holds
VH_DEV u32 trim_from(u32 v, int delta) { return lane_from(v, delta); }
VH_DEV f64 trim_from(f64 v, int delta)
{
	const u64 bits = __builtin_bit_cast(u64, v);
	const u32 lo = lane_from((u32) bits, delta), hi = lane_from((u32) (bits >> 32), delta);
	return __builtin_bit_cast(f64, (u64) lo | ((u64) hi << 32));
}

// the wave's 64 values added by rotation: every lane ends with the sum, always in the same order
template <typename S>
VH_DEV S trim_wave_sum(S v)
{
#pragma unroll
	for (int delta = 32; delta > 0; delta >>= 1)
		v += trim_from(v, delta);
	return v;
}
VH_DEV u32 trim_wave_min(u32 v)
{
#pragma unroll
	for (int delta = 32; delta > 0; delta >>= 1) {
		const u32 o = lane_from(v, delta);
		v = o < v ? o : v;
	}
	return v;
}
VH_DEV u32 trim_wave_max(u32 v)
{
#pragma unroll
	for (int delta = 32; delta > 0; delta >>= 1) {
		const u32 o = lane_from(v, delta);
		v = o > v ? o : v;
	}
	return v;
}

// one add per block and output element
template <typename S>
VH_DEV void project_emit(void *out, f64 *part, size_t part_row, size_t index, S v)
{
	if constexpr (std::is_same<S, f64>::value)
		part[part_row + index] = v;
	else
		atomicAdd((u32 *) out + index, v);
}

// double sums: the block that takes the last ticket adds the slabs, rows in index order
template <typename S>
VH_DEV void project_finish(const ProjectArgs &a, int col_rows, int row_rows)
{
	if constexpr (std::is_same<S, f64>::value) {
		__shared__ u32 s_last;
		__threadfence(); // (this thread's partials, before the ticket)
		barrier();
		if (tid() == 0) {
			const u32 blocks = gridDim.x * gridDim.y * gridDim.z;
			s_last = atomicAdd(a.ticket, 1u) == blocks - 1 ? 1u : 0u;
		}
		barrier();
		if (!s_last)
			return;
		__threadfence();
		const size_t n_rows = (size_t) a.height * a.bands;
		for (size_t i = (size_t) tid(); i < (size_t) a.elems; i += TRIM_THREADS) {
			f64 sum = 0.0;
			for (int k = 0; k < col_rows; k++)
				sum += __builtin_bit_cast(f64, VH_LOAD_SYS((u64 *) a.col_part + (size_t) k * a.elems + i));
			((f64 *) a.columns)[i] = sum;
		}
		for (size_t i = (size_t) tid(); i < n_rows; i += TRIM_THREADS) {
			f64 sum = 0.0;
			for (int k = 0; k < row_rows; k++)
				sum += __builtin_bit_cast(f64, VH_LOAD_SYS((u64 *) a.row_part + (size_t) k * n_rows + i));
			((f64 *) a.rows)[i] = sum;
		}
	}
}

// ---------------------------------------------------------------- project, 16 bytes a lane

template <typename T, int B>
__global__ void __launch_bounds__(TRIM_THREADS)
project_stream_kernel(ProjectArgs a)
{
	typedef typename ProjectSum<T>::type S;
	constexpr int NE = TRIM_GROUP / (int) sizeof(T);
	__shared__ S s_rows[TRIM_ROWS][TRIM_WAVES][B];

	const int t = tid();
	const int wave = t >> 6;
	const long long e0l = ((long long) blockIdx.x * TRIM_THREADS + t) * NE;
	const int n = e0l >= a.elems ? 0 : a.elems - (int) e0l < NE ? a.elems - (int) e0l : NE; // elements of the row this lane owns
	const int e0 = n ? (int) e0l : 0;
	const int b0 = e0 % B; // the band of the lane's first element
	const size_t n_rows = (size_t) a.height * B;

	S col[NE];
#pragma unroll
	for (int j = 0; j < NE; j++)
		col[j] = 0;

	for (int y0 = (int) blockIdx.y * TRIM_ROWS; y0 < a.height; y0 += (int) gridDim.y * TRIM_ROWS) {
		const int rows = min(TRIM_ROWS, a.height - y0);
		for (int r0 = 0; r0 < rows; r0 += TRIM_AHEAD) {
			// the loads of TRIM_AHEAD rows are in flight before the first of them is added up
			unsigned int d[TRIM_AHEAD][4];
#pragma unroll
			for (int q = 0; q < TRIM_AHEAD; q++) {
#pragma unroll
				for (int i = 0; i < 4; i++)
					d[q][i] = 0;
				if (r0 + q < rows) {
					const unsigned long long row = (unsigned long long) a.in + (unsigned long long) (y0 + r0 + q) * (unsigned long long) a.stride;
					if (n == NE)
						gload128(gptr_in_of(row), (unsigned int) e0 * (unsigned int) sizeof(T), d[q]);
					else {
						// the row's ragged last group, element by element (nothing past the row's last element is read)
#pragma unroll
						for (int j = 0; j < NE; j++)
							if (j < n)
								group_put<T>(d[q], j, ((const T *) row)[e0 + j]);
					}
				}
			}
#pragma unroll
			for (int q = 0; q < TRIM_AHEAD; q++) {
				if (r0 + q >= rows)
					break;
				S rel[B]; // rel[k]: the lane's elements of band (b0 + k) mod B
#pragma unroll
				for (int k = 0; k < B; k++)
					rel[k] = 0;
#pragma unroll
				for (int j = 0; j < NE; j++) {
					const S v = project_value<T>(group_take<T, 4>(d[q], j)); // (what lies past the row is zero)
					col[j] += v;
					rel[j % B] += v;
				}
#pragma unroll
				for (int b = 0; b < B; b++) {
					S v = rel[0]; // (b0 == b)
#pragma unroll
					for (int k = 1; k < B; k++)
						v = (b0 + k) % B == b ? rel[k] : v;
					v = trim_wave_sum<S>(v);
					if ((t & 63) == 0)
						s_rows[r0 + q][wave][b] = v;
				}
			}
		}
		barrier();
		if (t < rows * B) {
			const int r = t / B, b = t - r * B;
			S v = s_rows[r][0][b];
#pragma unroll
			for (int w = 1; w < TRIM_WAVES; w++)
				v += s_rows[r][w][b];
			project_emit<S>(a.rows, a.row_part, (size_t) blockIdx.x * n_rows, (size_t) (y0 + r) * B + b, v);
		}
		barrier();
	}
#pragma unroll
	for (int j = 0; j < NE; j++)
		if (j < n)
			project_emit<S>(a.columns, a.col_part, (size_t) blockIdx.y * a.elems, (size_t) (e0 + j), col[j]);
	project_finish<S>(a, (int) gridDim.y, (int) gridDim.x);
}

// ---------------------------------------------------------------- project, one element a lane

template <typename T>
__global__ void __launch_bounds__(TRIM_THREADS)
project_general_kernel(ProjectArgs a)
{
	typedef typename ProjectSum<T>::type S;
	__shared__ S s_rows[TRIM_ROWS][TRIM_WAVES];

	const int t = tid();
	const int wave = t >> 6;
	const int band = (int) blockIdx.z;
	const long long xl = (long long) blockIdx.x * TRIM_THREADS + t;
	const bool inside = xl < a.width;
	const size_t e = inside ? (size_t) xl * a.bands + band : 0;
	const size_t n_rows = (size_t) a.height * a.bands;

	S col = 0;
	for (int y0 = (int) blockIdx.y * TRIM_ROWS; y0 < a.height; y0 += (int) gridDim.y * TRIM_ROWS) {
		const int rows = min(TRIM_ROWS, a.height - y0);
		for (int r = 0; r < rows; r++) {
			S v = 0;
			if (inside)
				v = project_value<T>(((const T *) (a.in + (long long) (y0 + r) * a.stride))[e]);
			col += v;
			v = trim_wave_sum<S>(v);
			if ((t & 63) == 0)
				s_rows[r][wave] = v;
		}
		barrier();
		if (t < rows) {
			S v = s_rows[t][0];
#pragma unroll
			for (int w = 1; w < TRIM_WAVES; w++)
				v += s_rows[t][w];
			project_emit<S>(a.rows, a.row_part, (size_t) blockIdx.x * n_rows, (size_t) (y0 + t) * a.bands + band, v);
		}
		barrier();
	}
	if (inside)
		project_emit<S>(a.columns, a.col_part, (size_t) blockIdx.y * a.elems, e, col);
	project_finish<S>(a, (int) gridDim.y, (int) gridDim.x);
}

// ---------------------------------------------------------------- profile

struct ProfileArgs {
	const unsigned char *in;
	int *columns, *rows; // filled with height / width before the launch
	long long stride;    // bytes
	int width, height, bands;
};

template <typename T>
__global__ void __launch_bounds__(TRIM_THREADS)
profile_kernel(ProfileArgs a)
{
	__shared__ u32 s_rows[TRIM_ROWS][TRIM_WAVES];

	const int t = tid();
	const int wave = t >> 6;
	const int band = (int) blockIdx.z;
	const long long xl = (long long) blockIdx.x * TRIM_THREADS + t;
	const bool inside = xl < a.width;
	const size_t e = inside ? (size_t) xl * a.bands + band : 0;

	u32 first = (u32) a.height; // the first y at which the lane's element is non-zero
	for (int y0 = (int) blockIdx.y * TRIM_ROWS; y0 < a.height; y0 += (int) gridDim.y * TRIM_ROWS) {
		const int rows = min(TRIM_ROWS, a.height - y0);
		for (int r = 0; r < rows; r++) {
			bool set = false;
			if (inside)
				set = ((const T *) (a.in + (long long) (y0 + r) * a.stride))[e] != (T) 0; // profile.c:195 `if (p[j])`
			const u32 y = (u32) (y0 + r);
			first = set && y < first ? y : first;
			const u32 x = trim_wave_min(set ? (u32) xl : (u32) a.width);
			if ((t & 63) == 0)
				s_rows[r][wave] = x;
		}
		barrier();
		if (t < rows) {
			u32 x = s_rows[t][0];
#pragma unroll
			for (int w = 1; w < TRIM_WAVES; w++)
				x = s_rows[t][w] < x ? s_rows[t][w] : x;
			if (x < (u32) a.width)
				atomicMin(a.rows + (size_t) (y0 + t) * a.bands + band, (int) x);
		}
		barrier();
	}
	if (inside && first < (u32) a.height)
		atomicMin(a.columns + e, (int) first);
}

// ---------------------------------------------------------------- find_trim, fused

struct TrimFusedArgs {
	NbArgs nb;                 // the whole image as the input window and the output rect; `out` is not used
	const unsigned char *table; // device memory: 256 * bands bytes, table[band * 256 + value] != 0: the predicate holds
	u32 *bounds;               // width - min x, max x + 1, height - min y, max y + 1 of the set pels; zero before the launch
};

VH_DEV u32 trim_pk_min(u32 a, u32 b)
{
	typedef unsigned short us2 __attribute__((ext_vector_type(2)));
	return __builtin_bit_cast(u32, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
VH_DEV u32 trim_pk_max(u32 a, u32 b)
{
	typedef unsigned short us2 __attribute__((ext_vector_type(2)));
	return __builtin_bit_cast(u32, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
VH_DEV void trim_pk_sort2(u32 &a, u32 &b)
{
	const u32 lo = trim_pk_min(a, b), hi = trim_pk_max(a, b);
	a = lo;
	b = hi;
}
VH_DEV u32 trim_pk_med3(u32 a, u32 b, u32 c) { return trim_pk_max(trim_pk_min(a, b), trim_pk_min(trim_pk_max(a, b), c)); }

constexpr int TRIM_PK_ROWS = TRIM_FUSED_TH / (TRIM_THREADS / (TRIM_FUSED_TW / 4)); // output rows a lane makes: 2

template <bool MEDIAN>
__global__ void __launch_bounds__(TRIM_THREADS)
trim_fused_kernel(TrimFusedArgs a)
{
	VH_DYNAMIC_LDS(unsigned int, lds);
	__shared__ unsigned int s_table[256 + 64]; // 256 * 4 bytes, and 256 zero bytes for elements past the row's end
	__shared__ u32 s_bounds[4][TRIM_WAVES];
	static_assert(TRIM_PK_ROWS == 2, "a lane sorts four staged rows for two output rows");
	const NbArgs &nb = a.nb;

	const int t = tid();
	// (rows start on dwords or not: the table is bytes)
	{
		u32 w = 0;
		if (t < 64 * nb.bands)
			w = (u32) a.table[4 * t] | ((u32) a.table[4 * t + 1] << 8) | ((u32) a.table[4 * t + 2] << 16) | ((u32) a.table[4 * t + 3] << 24);
		s_table[t] = w;
		if (t < 64)
			s_table[256 + t] = 0;
	}
	const unsigned char *table = (const unsigned char *) s_table;

	const int out_e0 = (int) blockIdx.x * TRIM_FUSED_TW;
	const int s = out_e0 - nb.bands;
	const int s_al = s & ~3;
	const int lead = s - s_al;
	const int cx = t & (TRIM_FUSED_TW / 4 - 1), rg = t / (TRIM_FUSED_TW / 4);
	const int e = out_e0 + 4 * cx; // the lane's first element of the row
	const int out_elems = nb.out_width * nb.bands;
	const int row_dwords = nb.lds_row >> 2;

	// the pel and the band of the lane's four elements; wx: width - x, x1: x + 1 (0: the element lies past the row)
	u32 tab[4], wx[4], x1[4];
#pragma unroll
	for (int b = 0; b < 4; b++) {
		const int ee = e + b;
		const int pel = ee / nb.bands;
		tab[b] = ee < out_elems ? (u32) (ee - pel * nb.bands) * 256u : 1024u;
		wx[b] = ee < out_elems ? (u32) (nb.out_width - pel) : 0u;
		x1[b] = ee < out_elems ? (u32) (pel + 1) : 0u;
	}

	// hits: byte b is non-zero once element b of the lane's four has met its predicate in some row; below, above:
	// height - y and y + 1 of such rows
	u32 hits = 0, below = 0, above = 0;
	for (int tile = 0; tile < TRIM_FUSED_TILES; tile++) {
		const int y0 = ((int) blockIdx.y * TRIM_FUSED_TILES + tile) * TRIM_FUSED_TH;
		if (y0 >= nb.out_height)
			break;
		barrier(); // (the table is in place; the tile before this one has been read)
		nb_stage<1, false>(nb, lds, s_al, y0 - 1, TRIM_FUSED_TH + 2, TRIM_THREADS);
		barrier();

		u32 med[TRIM_PK_ROWS];
		if constexpr (MEDIAN) {
			// [0]: the even bytes of the lane's four elements, [1]: the odd ones; sorted along the staged row
			u32 lo[2][TRIM_PK_ROWS + 2], mid[2][TRIM_PK_ROWS + 2], hi[2][TRIM_PK_ROWS + 2];
#pragma unroll
			for (int r = 0; r < TRIM_PK_ROWS + 2; r++) {
				const unsigned int *row = lds + (TRIM_PK_ROWS * rg + r) * row_dwords + cx;
				u32 v[3];
#pragma unroll
				for (int i = 0; i < 3; i++) {
					const int o = lead + i * nb.bands;
					const u64 both = ((u64) row[(o >> 2) + 1] << 32) | row[o >> 2];
					v[i] = (u32) (both >> (8 * (o & 3)));
				}
#pragma unroll
				for (int h = 0; h < 2; h++) {
					u32 p = (v[0] >> (8 * h)) & 0x00ff00ffu, q = (v[1] >> (8 * h)) & 0x00ff00ffu, w = (v[2] >> (8 * h)) & 0x00ff00ffu;
					trim_pk_sort2(p, q);
					trim_pk_sort2(q, w);
					trim_pk_sort2(p, q);
					lo[h][r] = p;
					mid[h][r] = q;
					hi[h][r] = w;
				}
			}
#pragma unroll
			for (int k = 0; k < TRIM_PK_ROWS; k++) {
				u32 half[2];
#pragma unroll
				for (int h = 0; h < 2; h++)
					half[h] = trim_pk_med3(trim_pk_max(trim_pk_max(lo[h][k], lo[h][k + 1]), lo[h][k + 2]),
						trim_pk_med3(mid[h][k], mid[h][k + 1], mid[h][k + 2]), trim_pk_min(trim_pk_min(hi[h][k], hi[h][k + 1]), hi[h][k + 2]));
				med[k] = half[0] | (half[1] << 8);
			}
		}
		else {
#pragma unroll
			for (int k = 0; k < TRIM_PK_ROWS; k++) {
				const unsigned int *row = lds + (TRIM_PK_ROWS * rg + k + 1) * row_dwords + cx;
				const int o = lead + nb.bands;
				const u64 both = ((u64) row[(o >> 2) + 1] << 32) | row[o >> 2];
				med[k] = (u32) (both >> (8 * (o & 3)));
			}
		}
#pragma unroll
		for (int k = 0; k < TRIM_PK_ROWS; k++) {
			const int y = y0 + TRIM_PK_ROWS * rg + k;
			u32 row_hits = 0;
#pragma unroll
			for (int b = 0; b < 4; b++)
				row_hits |= (u32) table[tab[b] + ((med[k] >> (8 * b)) & 0xffu)] << (8 * b);
			// (a row past the image's last is made of copies of the last one: its medians are not the image's)
			row_hits = y < nb.out_height ? row_hits : 0u;
			hits |= row_hits;
			const bool set = row_hits != 0;
			below = set && (u32) (nb.out_height - y) > below ? (u32) (nb.out_height - y) : below;
			above = set && (u32) (y + 1) > above ? (u32) (y + 1) : above;
		}
	}
	u32 best[4] = { 0, 0, below, above };
#pragma unroll
	for (int b = 0; b < 4; b++) {
		const bool set = ((hits >> (8 * b)) & 0xffu) != 0;
		best[0] = set && wx[b] > best[0] ? wx[b] : best[0];
		best[1] = set && x1[b] > best[1] ? x1[b] : best[1];
	}
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const u32 v = trim_wave_max(best[i]);
		if ((t & 63) == 0)
			s_bounds[i][t >> 6] = v;
	}
	barrier();
	if (t < 4) {
		u32 v = s_bounds[t][0];
#pragma unroll
		for (int w = 1; w < TRIM_WAVES; w++)
			v = s_bounds[t][w] > v ? s_bounds[t][w] : v;
		// the result so far, past the caches: it only grows, so an old value costs an atomic and never a bound
		if (v > VH_LOAD_SYS(a.bounds + t))
			atomicMax(a.bounds + t, v);
	}
}

// ---------------------------------------------------------------- launches

static int trim_grid_y(long long blocks_x, int height)
{
	long long y = (height + TRIM_ROWS - 1) / TRIM_ROWS;
	const long long cap = blocks_x >= TRIM_GRID_BLOCKS ? 1 : TRIM_GRID_BLOCKS / blocks_x;
	y = y > cap ? cap : y;
	return (int) (y < 1 ? 1 : y);
}

static bool project_streams(const _VipsHipImage *in)
{
	if (getenv("VIPS_HIP_NO_TRIM_STREAM") || in->bands > 4)
		return false;
	return ((uintptr_t) in->data | (uintptr_t) in->stride) % 4 == 0;
}

void project_grid(const _VipsHipImage *in, int grid[3])
{
	if (project_streams(in)) {
		const long long groups = ((long long) in->width * in->bands * format_sizeof(in->format) + TRIM_GROUP - 1) / TRIM_GROUP;
		grid[0] = (int) ((groups + TRIM_THREADS - 1) / TRIM_THREADS);
		grid[1] = trim_grid_y(grid[0], in->height);
		grid[2] = 1;
	}
	else {
		grid[0] = (in->width + TRIM_THREADS - 1) / TRIM_THREADS;
		grid[1] = trim_grid_y((long long) grid[0] * in->bands, in->height);
		grid[2] = in->bands;
	}
}

static int trim_check_image(const char *domain, const _VipsHipImage *in)
{
	if (in->width < 1 || in->height < 1 || in->bands < 1 || in->bands > 65535 ||
		(long long) in->width * in->bands * format_sizeof(in->format) >= (1LL << 31) || (long long) in->height * in->bands >= (1LL << 31)) {
		error(domain, "image too large");
		return -1;
	}
	if (((uintptr_t) in->data | (uintptr_t) in->stride) % (uintptr_t) format_sizeof(in->format)) {
		error(domain, "rows must start on whole elements");
		return -1;
	}
	return 0;
}

template <typename T>
static int project_launch(const char *domain, const _VipsHipImage *in, ProjectArgs a)
{
	int g[3];
	project_grid(in, g);
	const dim3 grid(g[0], g[1], g[2]), block(TRIM_THREADS, 1, 1);
	if (project_streams(in)) {
		Gate gate("project_stream");
		switch (in->bands) {
		case 1: hipLaunchKernelGGL((project_stream_kernel<T, 1>), grid, block, 0, stream(), a); break;
		case 2: hipLaunchKernelGGL((project_stream_kernel<T, 2>), grid, block, 0, stream(), a); break;
		case 3: hipLaunchKernelGGL((project_stream_kernel<T, 3>), grid, block, 0, stream(), a); break;
		default: hipLaunchKernelGGL((project_stream_kernel<T, 4>), grid, block, 0, stream(), a); break;
		}
	}
	else {
		Gate gate("project_general");
		hipLaunchKernelGGL((project_general_kernel<T>), grid, block, 0, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

// Everything has been checked (ops_trim.cpp).  Integer sums: `columns` and `rows` are zero.  Double sums: col_part holds
// grid[1] * elems doubles, row_part grid[0] * height * bands (project_grid), *ticket is zero.
int project_run(const char *domain, const _VipsHipImage *in, void *columns, void *rows, double *col_part, double *row_part,
	unsigned int *ticket)
{
	if (trim_check_image(domain, in))
		return -1;
	ProjectArgs a = {};
	a.in = (const unsigned char *) in->data;
	a.columns = columns;
	a.rows = rows;
	a.col_part = col_part;
	a.row_part = row_part;
	a.ticket = ticket;
	a.stride = (long long) in->stride;
	a.width = in->width;
	a.height = in->height;
	a.bands = in->bands;
	a.elems = in->width * in->bands;
	switch (in->format) {
	case VIPS_HIP_FORMAT_UCHAR: return project_launch<u8>(domain, in, a);
	case VIPS_HIP_FORMAT_CHAR: return project_launch<s8>(domain, in, a);
	case VIPS_HIP_FORMAT_USHORT: return project_launch<u16>(domain, in, a);
	case VIPS_HIP_FORMAT_SHORT: return project_launch<s16>(domain, in, a);
	case VIPS_HIP_FORMAT_UINT: return project_launch<u32>(domain, in, a);
	case VIPS_HIP_FORMAT_INT: return project_launch<s32>(domain, in, a);
	case VIPS_HIP_FORMAT_FLOAT: return project_launch<f32>(domain, in, a);
	case VIPS_HIP_FORMAT_DOUBLE: return project_launch<f64>(domain, in, a);
	default:
		error(domain, "no kernel for format %d", in->format);
		return -1;
	}
}

template <typename T>
static int profile_launch(const ProfileArgs &a)
{
	const int bx = (a.width + TRIM_THREADS - 1) / TRIM_THREADS;
	const dim3 grid(bx, trim_grid_y((long long) bx * a.bands, a.height), a.bands), block(TRIM_THREADS, 1, 1);
	Gate gate("profile");
	hipLaunchKernelGGL((profile_kernel<T>), grid, block, 0, stream(), a);
	VH_CHECK(hipGetLastError());
	return 0;
}

// `columns` holds width * bands ints of value height, `rows` height * bands ints of value width.
int profile_run(const char *domain, const _VipsHipImage *in, int *columns, int *rows)
{
	if (trim_check_image(domain, in))
		return -1;
	ProfileArgs a = {};
	a.in = (const unsigned char *) in->data;
	a.columns = columns;
	a.rows = rows;
	a.stride = (long long) in->stride;
	a.width = in->width;
	a.height = in->height;
	a.bands = in->bands;
	switch (in->format) {
	case VIPS_HIP_FORMAT_UCHAR: return profile_launch<u8>(a);
	case VIPS_HIP_FORMAT_CHAR: return profile_launch<s8>(a);
	case VIPS_HIP_FORMAT_USHORT: return profile_launch<u16>(a);
	case VIPS_HIP_FORMAT_SHORT: return profile_launch<s16>(a);
	case VIPS_HIP_FORMAT_UINT: return profile_launch<u32>(a);
	case VIPS_HIP_FORMAT_INT: return profile_launch<s32>(a);
	case VIPS_HIP_FORMAT_FLOAT: return profile_launch<f32>(a);
	case VIPS_HIP_FORMAT_DOUBLE: return profile_launch<f64>(a);
	default:
		error(domain, "no kernel for format %d", in->format);
		return -1;
	}
}

// a uchar image of 1 .. 4 bands; `table` 256 * bands bytes and `bounds` four zero dwords, both in device memory
int trim_fused_run(const char *domain, const _VipsHipImage *in, int median, const unsigned char *table, unsigned int *bounds)
{
	if (trim_check_image(domain, in))
		return -1;
	if (in->format != VIPS_HIP_FORMAT_UCHAR || in->bands > 4) {
		error(domain, "the fused kernel takes uchar images of 1 to 4 bands");
		return -1;
	}
	const long long elems = (long long) in->width * in->bands;
	const long long blocks_y = (in->height + TRIM_FUSED_TH * TRIM_FUSED_TILES - 1) / (TRIM_FUSED_TH * TRIM_FUSED_TILES);
	if (blocks_y > 65535) {
		error(domain, "image too large");
		return -1;
	}
	TrimFusedArgs a = {};
	a.nb.in = (const unsigned char *) in->data;
	a.nb.in_stride = (long long) in->stride;
	a.nb.in_width = a.nb.im_width = a.nb.out_width = in->width;
	a.nb.in_height = a.nb.im_height = a.nb.out_height = in->height;
	a.nb.bands = in->bands;
	a.nb.win_w = a.nb.win_h = 3;
	// bytes of a staged row: the lead of the rounding, the tile, the halo and the dword behind the last one a
	// byte-shifted read takes; whole 16-byte groups (as rank.hip's)
	a.nb.lds_row = (3 + TRIM_FUSED_TW + 2 * in->bands + 4 + 15) / 16 * 16;
	a.table = table;
	a.bounds = bounds;
	const dim3 grid((unsigned int) ((elems + TRIM_FUSED_TW - 1) / TRIM_FUSED_TW), (unsigned int) blocks_y, 1), block(TRIM_THREADS, 1, 1);
	const size_t lds = (size_t) (TRIM_FUSED_TH + 2) * a.nb.lds_row;
	Gate gate("trim_fused");
	if (median)
		hipLaunchKernelGGL((trim_fused_kernel<true>), grid, block, lds, stream(), a);
	else
		hipLaunchKernelGGL((trim_fused_kernel<false>), grid, block, lds, stream(), a);
	VH_CHECK(hipGetLastError());
	return 0;
}

int trim_tile(int what)
{
	switch (what) {
	case 0: return TRIM_THREADS;
	case 1: return TRIM_GROUP;
	case 2: return TRIM_FUSED_TH;
	case 3: return TRIM_GRID_BLOCKS;
	case 4: return TRIM_FUSED_TW;
	case 5: return TRIM_FUSED_TH * TRIM_FUSED_TILES;
	case 6: return TRIM_ROWS;
	default: return 0;
	}
}

} // namespace vh
