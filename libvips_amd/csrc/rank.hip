// vips_rank (morphology/rank.c): the index-th smallest element of a width x height window, band by band, on the
// device (gfx950).  The reference picks one of four routes (a uchar histogram walk, a max loop, a min loop, a
// quickselect: rank.c:444-453, 491-503); all four give the same order statistic, and this file picks its own:
//
//   rank_median3   3 x 3, index 4.  Nine keys in registers, a min / max exchange network: each row of the window
//                  is sorted (3 exchanges), then med3(max of the lows, med3 of the mids, min of the highs).
//                  One-byte elements take a packed form of it (rank_median3_u8_kernel): a lane owns a DWORD of two
//                  output rows, the three neighbours of a staged row are byte-shifted dword reads, the bytes are
//                  spread to two 16-bit halves a register (even and odd bytes) and every exchange is a packed
//                  16-bit min / max on two elements; the four sorted rows serve both output rows.
//   rank_minmax    index 0 or n - 1, any window: separable.  Pass 1 takes the minimum along every staged row into a
//                  second LDS plane, pass 2 takes the minimum down the columns of that plane.  A maximum is the
//                  minimum of the inverted keys.
//   rank_select    everything else: bisection on the key, from the top bit down.  A round asks how many keys of
//                  the window (in LDS) are >= the candidate; the candidate's bit stays when at least n - index
//                  are.  8, 16 or 32 rounds of n compares an output, and no private array (a per-lane sort[n] would
//                  live in scratch).
//
// All three work on order-preserving unsigned KEYS made while the tile is staged (nbhd_tile.h): signed formats
// have their sign bit flipped, floats take the usual flip (negative: all bits; else: the sign), so one kernel per
// element size (+ one for float) serves uchar, char, ushort, short, uint, int and float.  Float results are defined
// for inputs without NaN (a NaN's key sorts beyond the infinities; the reference's answer depends on its route) and
// compare equal by value (-0 sorts below +0 here).  Double and complex images are refused by the host.
//
// Geometry: a block of 256 threads makes RANK_TW = 256 elements x RANK_TH = 8 rows; thread t owns column t.  The
// window's size is limited by LDS alone: (8 + height - 1) staged rows (+ as many rows of 256 keys for rank_minmax)
// must fit RANK_LDS_MAX = 160 KB, a CU's whole LDS -- 31 x 31 fits for every format up to 16 bands; the host refuses
// what does not.
#include "nbhd_tile.h"

#include <cstdint>

namespace vh {

constexpr int RANK_THREADS = 256;
constexpr int RANK_TW = 256; // elements
constexpr int RANK_TH = 8;   // rows
constexpr int RANK_LDS_MAX = 160 * 1024; // a CU's LDS: one block a CU at the largest windows

enum { RANK_ALG_MEDIAN3 = 0, RANK_ALG_MINMAX = 1, RANK_ALG_SELECT = 2 };

template <int ES>
struct RankKey;
template <>
struct RankKey<1> {
	typedef unsigned char type;
};
template <>
struct RankKey<2> {
	typedef unsigned short type;
};
template <>
struct RankKey<4> {
	typedef unsigned int type;
};

VH_DEV unsigned int rank_min(unsigned int a, unsigned int b) { return a < b ? a : b; }
VH_DEV unsigned int rank_max(unsigned int a, unsigned int b) { return a > b ? a : b; }
VH_DEV void rank_sort2(unsigned int &a, unsigned int &b)
{
	const unsigned int lo = rank_min(a, b), hi = rank_max(a, b);
	a = lo;
	b = hi;
}
VH_DEV unsigned int rank_med3(unsigned int a, unsigned int b, unsigned int c)
{
	return rank_max(rank_min(a, b), rank_min(rank_max(a, b), c));
}

template <int ES, bool KEYF>
VH_DEV void rank_store(const NbArgs &a, int y, int e, unsigned int key)
{
	const unsigned int v = nb_unkey<KEYF>(key, a.key_xor);
	const gptr_out p = gptr_out_of((unsigned long long) a.out + (unsigned long long) y * (unsigned long long) a.out_stride +
		(unsigned long long) e * ES);
	if constexpr (ES == 1)
		gstore8(p, (unsigned char) v);
	else if constexpr (ES == 2)
		gstore16(p, (unsigned short) v);
	else
		gstore32(p, v);
}

template <int ES, bool KEYF, int ALG>
__global__ void __launch_bounds__(RANK_THREADS)
rank_kernel(NbArgs a)
{
	typedef typename RankKey<ES>::type K;
	VH_DYNAMIC_LDS(unsigned int, lds);
	constexpr int ALIGN = 4 / ES; // elements a dword

	const int out_e0 = a.out_left * a.bands + (int) blockIdx.x * RANK_TW; // the tile's first element, of the image row
	const int y0 = (int) blockIdx.y * RANK_TH;                             // the tile's first row, of the output rect
	const int s = out_e0 - (a.win_w / 2) * a.bands;
	const int s_al = s & ~(ALIGN - 1); // (rounds down for negative s too)
	const int lead = s - s_al;
	const int rows = RANK_TH + a.win_h - 1;
	nb_stage<ES, KEYF>(a, lds, s_al, a.out_top + y0 - a.win_h / 2, rows, RANK_THREADS);
	barrier();

	const int t = tid();
	const int e = (int) blockIdx.x * RANK_TW + t; // of the output rect's row
	const bool inside = e < a.out_width * a.bands;
	const int row_keys = a.lds_row / ES;
	const K *keys = (const K *) lds + lead + t;

	if constexpr (ALG == RANK_ALG_MEDIAN3) {
		for (int ty = 0; ty < RANK_TH; ty++) {
			if (y0 + ty >= a.out_height)
				break;
			unsigned int lo[3], mid[3], hi[3];
#pragma unroll
			for (int j = 0; j < 3; j++) {
				const K *row = keys + (ty + j) * row_keys;
				unsigned int p = row[0], q = row[a.bands], r = row[2 * a.bands];
				rank_sort2(p, q);
				rank_sort2(q, r);
				rank_sort2(p, q);
				lo[j] = p;
				mid[j] = q;
				hi[j] = r;
			}
			const unsigned int v = rank_med3(rank_max(rank_max(lo[0], lo[1]), lo[2]), rank_med3(mid[0], mid[1], mid[2]),
				rank_min(rank_min(hi[0], hi[1]), hi[2]));
			if (inside)
				rank_store<ES, KEYF>(a, y0 + ty, e, v);
		}
	}
	else if constexpr (ALG == RANK_ALG_MINMAX) {
		K *plane = (K *) ((unsigned char *) lds + rows * a.lds_row) + t; // rows x RANK_TW keys
		for (int r = 0; r < rows; r++) {
			const K *row = keys + r * row_keys;
			unsigned int m = row[0];
			for (int i = 1; i < a.win_w; i++)
				m = rank_min(m, row[i * a.bands]);
			plane[r * RANK_TW] = (K) m;
		}
		barrier();
		for (int ty = 0; ty < RANK_TH; ty++) {
			if (y0 + ty >= a.out_height)
				break;
			unsigned int m = plane[ty * RANK_TW];
			for (int j = 1; j < a.win_h; j++)
				m = rank_min(m, plane[(ty + j) * RANK_TW]);
			if (inside)
				rank_store<ES, KEYF>(a, y0 + ty, e, m);
		}
	}
	else {
		const int need = a.win_w * a.win_h - a.index; // keys >= the answer
		for (int ty = 0; ty < RANK_TH; ty++) {
			if (y0 + ty >= a.out_height)
				break;
			unsigned int v = 0;
			for (int bit = 8 * ES - 1; bit >= 0; bit--) {
				const unsigned int cand = v | (1u << bit);
				int count = 0;
				for (int j = 0; j < a.win_h; j++) {
					const K *row = keys + (ty + j) * row_keys;
					for (int i = 0; i < a.win_w; i++)
						count += row[i * a.bands] >= cand ? 1 : 0;
				}
				v = count >= need ? cand : v;
			}
			if (inside)
				rank_store<ES, KEYF>(a, y0 + ty, e, v);
		}
	}
}

// ---- rank_median3 on packed bytes: two elements a register half-pair
typedef unsigned short rank_us2 __attribute__((ext_vector_type(2)));
VH_DEV unsigned int rank_pk_min(unsigned int a, unsigned int b)
{
	return __builtin_bit_cast(unsigned int, __builtin_elementwise_min(__builtin_bit_cast(rank_us2, a), __builtin_bit_cast(rank_us2, b)));
}
VH_DEV unsigned int rank_pk_max(unsigned int a, unsigned int b)
{
	return __builtin_bit_cast(unsigned int, __builtin_elementwise_max(__builtin_bit_cast(rank_us2, a), __builtin_bit_cast(rank_us2, b)));
}
VH_DEV void rank_pk_sort2(unsigned int &a, unsigned int &b)
{
	const unsigned int lo = rank_pk_min(a, b), hi = rank_pk_max(a, b);
	a = lo;
	b = hi;
}
VH_DEV unsigned int rank_pk_med3(unsigned int a, unsigned int b, unsigned int c)
{
	return rank_pk_max(rank_pk_min(a, b), rank_pk_min(rank_pk_max(a, b), c));
}

constexpr int RANK_PK_ROWS = RANK_TH / (RANK_THREADS / (RANK_TW / 4)); // output rows a lane makes: 2

__global__ void __launch_bounds__(RANK_THREADS)
rank_median3_u8_kernel(NbArgs a)
{
	VH_DYNAMIC_LDS(unsigned int, lds);
	static_assert(RANK_PK_ROWS == 2, "a lane sorts four staged rows for two output rows");

	const int out_e0 = a.out_left * a.bands + (int) blockIdx.x * RANK_TW;
	const int y0 = (int) blockIdx.y * RANK_TH;
	const int s = out_e0 - a.bands;
	const int s_al = s & ~3;
	const int lead = s - s_al;
	nb_stage<1, false>(a, lds, s_al, a.out_top + y0 - 1, RANK_TH + 2, RANK_THREADS);
	barrier();

	const int t = tid();
	const int cx = t & (RANK_TW / 4 - 1), rg = t / (RANK_TW / 4);
	const int e = (int) blockIdx.x * RANK_TW + 4 * cx; // the lane's first element, of the output rect's row
	const int out_elems = a.out_width * a.bands;
	const int row_dwords = a.lds_row >> 2;

	// [0]: the even bytes of the lane's four elements, [1]: the odd ones; sorted along the staged row
	unsigned int lo[2][RANK_PK_ROWS + 2], mid[2][RANK_PK_ROWS + 2], hi[2][RANK_PK_ROWS + 2];
#pragma unroll
	for (int r = 0; r < RANK_PK_ROWS + 2; r++) {
		const unsigned int *row = lds + (RANK_PK_ROWS * rg + r) * row_dwords + cx;
		unsigned int v[3];
#pragma unroll
		for (int i = 0; i < 3; i++) {
			const int o = lead + i * a.bands;
			const unsigned long long both = ((unsigned long long) row[(o >> 2) + 1] << 32) | row[o >> 2];
			v[i] = (unsigned int) (both >> (8 * (o & 3)));
		}
#pragma unroll
		for (int h = 0; h < 2; h++) {
			unsigned int p = (v[0] >> (8 * h)) & 0x00ff00ffu, q = (v[1] >> (8 * h)) & 0x00ff00ffu, w = (v[2] >> (8 * h)) & 0x00ff00ffu;
			rank_pk_sort2(p, q);
			rank_pk_sort2(q, w);
			rank_pk_sort2(p, q);
			lo[h][r] = p;
			mid[h][r] = q;
			hi[h][r] = w;
		}
	}
#pragma unroll
	for (int k = 0; k < RANK_PK_ROWS; k++) {
		const int y = y0 + RANK_PK_ROWS * rg + k;
		unsigned int half[2];
#pragma unroll
		for (int h = 0; h < 2; h++)
			half[h] = rank_pk_med3(rank_pk_max(rank_pk_max(lo[h][k], lo[h][k + 1]), lo[h][k + 2]),
				rank_pk_med3(mid[h][k], mid[h][k + 1], mid[h][k + 2]), rank_pk_min(rank_pk_min(hi[h][k], hi[h][k + 1]), hi[h][k + 2]));
		const unsigned int v = (half[0] | (half[1] << 8)) ^ a.key_xor;
		if (y < a.out_height && e < out_elems) {
			const unsigned long long p = (unsigned long long) a.out + (unsigned long long) y * (unsigned long long) a.out_stride +
				(unsigned long long) e;
			if ((p & 3) == 0 && e + 4 <= out_elems)
				gstore32(gptr_out_of(p), v);
			else {
#pragma unroll
				for (int b = 0; b < 4; b++)
					if (e + b < out_elems)
						gstore8(gptr_out_of(p + b), (unsigned char) (v >> (8 * b)));
			}
		}
	}
}

// bytes of a staged row for a window `win_w` wide: the lead of the rounding, the tile, the halo (and the dword behind
// the last one a byte-shifted read takes); whole 16-byte groups
static int rank_lds_row(int es, int bands, int win_w)
{
	const long long bytes = ((long long) (4 / es - 1) + RANK_TW + (long long) (win_w - 1) * bands) * es + 4;
	const long long row = (bytes + 15) / 16 * 16;
	return row > RANK_LDS_MAX ? RANK_LDS_MAX + 16 : (int) row;
}

template <typename K>
static int rank_launch(K kernel, const char *gate_name, const NbArgs &a, dim3 grid, size_t lds)
{
	if (lds > 64 * 1024)
		VH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, RANK_LDS_MAX));
	Gate gate(gate_name);
	hipLaunchKernelGGL(kernel, grid, dim3(RANK_THREADS), lds, stream(), a);
	VH_CHECK(hipGetLastError());
	return 0;
}

template <int ES, bool KEYF>
static int rank_go(int alg, const NbArgs &a, dim3 grid, size_t lds)
{
	switch (alg) {
	case RANK_ALG_MEDIAN3:
		if constexpr (ES == 1)
			return rank_launch(rank_median3_u8_kernel, "rank_median3", a, grid, lds);
		else
			return rank_launch(rank_kernel<ES, KEYF, RANK_ALG_MEDIAN3>, "rank_median3", a, grid, lds);
	case RANK_ALG_MINMAX:
		return rank_launch(rank_kernel<ES, KEYF, RANK_ALG_MINMAX>, "rank_minmax", a, grid, lds);
	default:
		return rank_launch(rank_kernel<ES, KEYF, RANK_ALG_SELECT>, "rank_select", a, grid, lds);
	}
}

// Everything about the regions has been checked (ops_morphology.cpp); `format` is one of uchar .. float.
int rank_run(const char *domain, NbArgs a, int format)
{
	const int es = format_sizeof(format);
	const int n = a.win_w * a.win_h;
	const bool extreme = a.index == 0 || a.index == n - 1;
	const int alg = extreme ? RANK_ALG_MINMAX : a.win_w == 3 && a.win_h == 3 && a.index == 4 ? RANK_ALG_MEDIAN3 : RANK_ALG_SELECT;

	a.lds_row = rank_lds_row(es, a.bands, a.win_w);
	const long long rows = RANK_TH + a.win_h - 1;
	const long long lds = rows * a.lds_row + (alg == RANK_ALG_MINMAX ? rows * RANK_TW * es : 0);
	if (lds > RANK_LDS_MAX) {
		error(domain, "a %d x %d window on %d-band images of %d-byte elements needs %lld KB of LDS, the kernel has %d",
			a.win_w, a.win_h, a.bands, es, (lds + 1023) / 1024, RANK_LDS_MAX / 1024);
		return -1;
	}
	// keys: unsigned order is the format's order; a maximum is the minimum of the inverted keys
	const bool is_signed = format == VIPS_HIP_FORMAT_CHAR || format == VIPS_HIP_FORMAT_SHORT || format == VIPS_HIP_FORMAT_INT;
	a.key_xor = !is_signed ? 0u : es == 1 ? 0x80808080u : es == 2 ? 0x80008000u : 0x80000000u;
	if (alg == RANK_ALG_MINMAX && a.index != 0) {
		a.key_xor ^= 0xffffffffu;
		a.index = 0;
	}
	const long long out_elems = (long long) a.out_width * a.bands;
	const dim3 grid((unsigned int) ((out_elems + RANK_TW - 1) / RANK_TW), (unsigned int) ((a.out_height + RANK_TH - 1) / RANK_TH), 1);
	if (format == VIPS_HIP_FORMAT_FLOAT)
		return rank_go<4, true>(alg, a, grid, (size_t) lds);
	return es == 1 ? rank_go<1, false>(alg, a, grid, (size_t) lds)
		: es == 2  ? rank_go<2, false>(alg, a, grid, (size_t) lds)
				   : rank_go<4, false>(alg, a, grid, (size_t) lds);
}

int rank_tile(int what)
{
	return what == 0 ? RANK_TW : what == 1 ? RANK_TH : 0;
}

} // namespace vh
