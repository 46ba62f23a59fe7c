// vips_arrayjoin, vips_replicate, vips_wrap and vips_grid (conversion/arrayjoin.c, replicate.c, wrap.c, grid.c) on the
// device (gfx950).
//
// The family is data movement over a lattice: the output is cut into cells of cell_w x cell_h pels, and a pel of a cell
// is a pel of ONE source row or the ink.  Output pel (X, Y) lies in cell (cx, cy) = ((X + org_x) / cell_w,
// (Y + org_y) / cell_h); cells_row() names the source row a cell shows on output row Y, where on the output that row's
// pel 0 lies, and how many pels it has (internal.h has the three ways to a cell's source: a table of descriptors, a
// period, a tile of a strip).  ONE launch an operation writes every byte of the rect once.
//
//   cells_stream<P>   lanes on consecutive 16-byte groups of an output row (48 for 3-, 6- and 12-byte pels), the rect's
//                     groups dealt to the lanes as one sequence, rows that start on dwords on every side.  A group
//                     whose pels lie in one cell and wholly inside its source columns is a source group that starts
//                     anywhere in the source row: the lane loads the aligned dwords round it (global_load_dwordx4, one
//                     dword more when the group is not dword aligned) and shifts them into place, as canvas_stream
//                     does; a group of one cell wholly off its source is the ink's bytes from the kernel's arguments,
//                     no load.  A group that straddles a cell edge or an image edge, or is the row's ragged end, goes
//                     pel by pel INSIDE the same kernel (byte loads, the cell looked up again only where it changes).
//                     Lanes of a wave mostly share a cell: the descriptor read is one or two cache lines a wave.
//   cells_general     one pel a lane, any pel size up to 32 bytes, any row alignment: defines correctness, takes rows
//                     that do not start on dwords, 24- and 32-byte pels, and everything under VIPS_HIP_NO_CELLS_STREAM.
//
// How global_load_dwordx4 / global_store_dwordx4 behave at addresses that are dword- but not 16-byte-aligned (a sheet
// whose row length is no multiple of 16) has not been measured on this part, here or for canvas.hip; nothing below
// assumes either answer.
#include "pointwise.h"

namespace vh {

constexpr int CELLS_THREADS = POINTWISE_THREADS;

constexpr int cells_group_of(int pel) { return 16 % pel == 0 ? 16 : (48 % pel == 0 ? 48 : 0); }

// byte i of the ink (i a constant once the loops are unrolled)
VH_DEV unsigned int cells_ink_byte(const CellsArgs &a, int i) { return (a.ink[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// what cell (cx, cy) shows on output row Y: the address of the source row's pel 0 (0: no row, the ink), the output
// column that pel lies at, the pels of the row
struct CellRow {
	unsigned long long row;
	int x0, w;
};

VH_DEV int cells_cx(const CellsArgs &a, int X) { return (int) ((unsigned int) (X + a.org_x) / (unsigned int) a.cell_w); }
VH_DEV int cells_cy(const CellsArgs &a, int Y) { return (int) ((unsigned int) (Y + a.org_y) / (unsigned int) a.cell_h); }

// two columns of cells show the same source (the table's clamp gives every cell past the last image the last image)
VH_DEV bool cells_same(const CellsArgs &a, int cxa, int cxb, int cy)
{
	if (a.mode == CELLS_TABLE)
		return min(a.n - 1, cxa + cy * a.across) == min(a.n - 1, cxb + cy * a.across);
	return cxa == cxb;
}

VH_DEV CellRow cells_row(const CellsArgs &a, int cx, int cy, int Y)
{
	CellRow r;
	if (a.mode == CELLS_TABLE) {
		const CellDesc d = a.table[min(a.n - 1, cx + cy * a.across)];
		const int v = Y - d.y0;
		r.x0 = d.x0;
		r.w = d.w;
		r.row = (unsigned int) v < (unsigned int) d.h ? (unsigned long long) d.base + (unsigned long long) v * d.stride : 0;
		return r;
	}
	int v = Y + a.org_y - cy * a.cell_h; // the row of the cell
	if (a.mode == CELLS_GRID)
		v += (cy * a.across + cx) * a.cell_h;
	r.x0 = cx * a.cell_w - a.org_x;
	r.w = a.cell_w;
	// (two's complement: the window's corner is taken off before any pel is addressed)
	r.row = (unsigned long long) a.src + (unsigned long long) ((long long) (v - a.win_top) * a.src_stride - (long long) a.win_left * a.pel);
	return r;
}

// where output pel X of a row comes from: its address, 0 for the ink
VH_DEV unsigned long long cells_pel(const CellsArgs &a, const CellRow &r, int X)
{
	const int u = X - r.x0;
	return r.row && (unsigned int) u < (unsigned int) r.w ? r.row + (unsigned long long) u * a.pel : 0;
}

// ---------------------------------------------------------------- one pel a lane

template <typename UT>
__global__ void __launch_bounds__(CELLS_THREADS)
cells_general_kernel(CellsArgs a)
{
	const int ox = (int) blockIdx.x * CELLS_THREADS + (int) threadIdx.x;
	if (ox >= a.out_width)
		return;
	const int units = a.pel / (int) sizeof(UT);
	const int X = a.out_left + ox, cx = cells_cx(a, X);
	for (int oy = (int) blockIdx.y; oy < a.out_height; oy += (int) gridDim.y) {
		const int Y = a.out_top + oy;
		const unsigned long long from = cells_pel(a, cells_row(a, cx, cells_cy(a, Y), Y), X);
		UT *dst = (UT *) (a.out + (long long) oy * a.out_stride + (long long) ox * a.pel);
		if (from) {
			const UT *src = (const UT *) from;
			for (int i = 0; i < units; i++)
				dst[i] = src[i];
		}
		else {
			for (int i = 0; i < units; i++) {
				UT v;
				if constexpr (sizeof(UT) == 8)
					v = (UT) a.ink[2 * i] | ((UT) a.ink[2 * i + 1] << 32);
				else
					v = (UT) (a.ink[i * (int) sizeof(UT) / 4] >> (8 * ((i * (int) sizeof(UT)) & 3)));
				dst[i] = v;
			}
		}
	}
}

// ---------------------------------------------------------------- 16 / 48 bytes a lane

template <int P>
__global__ void __launch_bounds__(CELLS_THREADS)
cells_stream_kernel(CellsArgs a)
{
	constexpr int NB = cells_group_of(P);
	constexpr int NP = NB / P, ND = NB / 4;
	// the rect's groups, rows after rows, dealt to the lanes as ONE sequence (as canvas_stream's)
	const unsigned int total = (unsigned int) a.groups * (unsigned int) a.out_height;
	for (unsigned int at = (unsigned int) blockIdx.x * CELLS_THREADS + (unsigned int) threadIdx.x; at < total; at += (unsigned int) gridDim.x * CELLS_THREADS) {
		const int y = (int) (at / (unsigned int) a.groups);
		const int g = (int) (at - (unsigned int) y * (unsigned int) a.groups);
		const int p0 = g * NP; // the group's first pel, in the rect
		const int X0 = a.out_left + p0, Y = a.out_top + y;
		const int npel = min(NP, a.out_width - p0); // < NP: the row's ragged end
		const bool whole = npel == NP;
		const int cy = cells_cy(a, Y), cx0 = cells_cx(a, X0);
		const gptr_out ob = gptr_out_of((unsigned long long) a.out + (unsigned long long) y * a.out_stride) + (unsigned int) g * NB;
		CellRow r = cells_row(a, cx0, cy, Y);
		unsigned int w[ND];
		unsigned long long src = 0;
		bool ink = false;
		if (whole && cells_same(a, cx0, cells_cx(a, X0 + NP - 1), cy)) {
			if (r.row && X0 >= r.x0 && X0 + NP <= r.x0 + r.w)
				src = r.row + (unsigned long long) (X0 - r.x0) * P;
			else if (!r.row || X0 + NP <= r.x0 || X0 >= r.x0 + r.w)
				ink = true;
		}
		if (src) {
			// the aligned dwords round the source group, shifted: rows start on dwords, so the last of them -- up to
			// 3 bytes past the group -- ends inside the source row's stride (an image's and a region's memory covers
			// height * stride)
			const unsigned int sh = (unsigned int) src & 3u;
			const gptr_in ib = gptr_in_of(src - sh);
			unsigned int d[ND + 1];
#pragma unroll
			for (int q = 0; q < ND / 4; q++) {
				unsigned int t[4];
				gload128(ib, 16 * q, t);
#pragma unroll
				for (int i = 0; i < 4; i++)
					d[4 * q + i] = t[i];
			}
			d[ND] = 0;
			if (sh)
				d[ND] = gload32(ib, NB);
#pragma unroll
			for (int i = 0; i < ND; i++)
				w[i] = (unsigned int) ((((unsigned long long) d[i + 1] << 32) | d[i]) >> (8 * sh));
		}
		else if (ink) {
#pragma unroll
			for (int i = 0; i < ND; i++)
				w[i] = cells_ink_byte(a, (4 * i) % P) | (cells_ink_byte(a, (4 * i + 1) % P) << 8) |
					(cells_ink_byte(a, (4 * i + 2) % P) << 16) | (cells_ink_byte(a, (4 * i + 3) % P) << 24);
		}
		else {
			// pel by pel: a cell edge or an image edge inside the group, the ragged end
#pragma unroll
			for (int i = 0; i < ND; i++)
				w[i] = 0;
			int cx = cx0;
#pragma unroll
			for (int j = 0; j < NP; j++) {
				if (j < npel) {
					const int c = cells_cx(a, X0 + j);
					if (c != cx) {
						cx = c;
						r = cells_row(a, cx, cy, Y);
					}
					const unsigned long long from = cells_pel(a, r, X0 + j);
#pragma unroll
					for (int b = 0; b < P; b++) {
						const int k = j * P + b;
						const unsigned int v = from ? (unsigned int) *(const unsigned char *) (from + b) : cells_ink_byte(a, b);
						w[k >> 2] |= v << (8 * (k & 3));
					}
				}
			}
		}
		if (whole) {
#pragma unroll
			for (int q = 0; q < ND / 4; q++) {
				const unsigned int t[4] = { w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3] };
				gstore128(ob + 16 * q, t);
			}
		}
		else {
#pragma unroll
			for (int k = 0; k < NB; k++)
				if (k < npel * P)
					gstore8(ob + k, (unsigned char) (w[k >> 2] >> (8 * (k & 3))));
		}
	}
}

// ---------------------------------------------------------------- dispatch

// the largest of 8, 4, 2, 1 that divides every row start (and the pel size)
static int cells_unit(const CellsArgs &a, unsigned long long starts, int most, bool with_pel)
{
	uintptr_t all = (uintptr_t) starts | (uintptr_t) a.out | (uintptr_t) a.out_stride;
	if (with_pel)
		all |= (uintptr_t) a.pel;
	int u = most;
	while (u > 1 && all % (uintptr_t) u)
		u >>= 1;
	return u;
}

static void cells_launch_general(const CellsArgs &a, unsigned long long starts)
{
	const int bx = (a.out_width + CELLS_THREADS - 1) / CELLS_THREADS;
	dim3 grid(bx, pointwise_rows_grid(bx, a.out_height), 1), block(CELLS_THREADS, 1, 1);
	Gate gate("cells_general");
	switch (cells_unit(a, starts, 8, true)) {
	case 8: hipLaunchKernelGGL((cells_general_kernel<unsigned long long>), grid, block, 0, stream(), a); break;
	case 4: hipLaunchKernelGGL((cells_general_kernel<unsigned int>), grid, block, 0, stream(), a); break;
	case 2: hipLaunchKernelGGL((cells_general_kernel<unsigned short>), grid, block, 0, stream(), a); break;
	default: hipLaunchKernelGGL((cells_general_kernel<unsigned char>), grid, block, 0, stream(), a); break;
	}
}

template <int P>
static void cells_launch_stream(CellsArgs a)
{
	constexpr int NP = cells_group_of(P) / P;
	a.groups = (a.out_width + NP - 1) / NP;
	dim3 grid = pointwise_stream_grid((long long) a.groups * a.out_height), block(CELLS_THREADS, 1, 1);
	Gate gate("cells_stream");
	hipLaunchKernelGGL((cells_stream_kernel<P>), grid, block, 0, stream(), a);
}

static bool cells_stream_ok(const CellsArgs &a, unsigned long long starts)
{
	if (getenv("VIPS_HIP_NO_CELLS_STREAM"))
		return false;
	// rows that start on dwords on every side: the aligned dwords round a source group then lie in its row
	if (a.pel > 16 || cells_group_of(a.pel) == 0 || cells_unit(a, starts, 4, false) != 4)
		return false;
	// (the kernel numbers the rect's groups in 32 bits)
	const long long groups = (a.out_width + (long long) cells_group_of(a.pel) / a.pel - 1) / (cells_group_of(a.pel) / a.pel);
	return groups * a.out_height < (1LL << 31);
}

int cells_tile(int what, int pel)
{
	switch (what) {
	case 0: return CELLS_THREADS;
	case 1: return pel >= 1 && pel <= 16 ? cells_group_of(pel) : 0;
	case 2: return POINTWISE_GRID_BLOCKS;
	default: return 0;
	}
}

int cells_run(const char *domain, CellsArgs a, unsigned long long starts)
{
	if (a.pel < 1 || a.pel > CANVAS_MAX_PEL) {
		error(domain, "pels of more than %d bytes are outside the HIP path", CANVAS_MAX_PEL);
		return -1;
	}
	// the kernels work out coordinates in int: with sizes and positions up to 10^9 every position + size, every
	// X + org and every row of a strip ((cy * across + cx) * cell_h + a row of the cell < sh) stays inside it
	constexpr int LIMIT = 1000000000;
	const int sizes[] = { a.cell_w, a.cell_h, a.out_width, a.out_height };
	for (int v : sizes)
		if (v < 1 || v > LIMIT) {
			error(domain, "image size out of range");
			return -1;
		}
	const int positions[] = { a.org_x, a.org_y, a.out_left, a.out_top, a.win_left, a.win_top, a.sw, a.sh };
	for (int v : positions)
		if (v < 0 || v > LIMIT) {
			error(domain, "position out of range");
			return -1;
		}
	const long long cells_down = ((long long) a.out_top + a.out_height + a.org_y + a.cell_h - 1) / a.cell_h;
	if (a.across < 0 || a.n < 0 || cells_down * a.across + a.across > LIMIT) {
		error(domain, "too many cells");
		return -1;
	}
	if ((long long) a.out_width * a.pel >= (1LL << 31) || (long long) a.cell_w * a.pel >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	if (cells_stream_ok(a, starts)) {
		switch (a.pel) {
#define GO(P) \
	case P: \
		cells_launch_stream<P>(a); \
		VH_CHECK(hipGetLastError()); \
		return 0;
			GO(1) GO(2) GO(3) GO(4) GO(6) GO(8) GO(12) GO(16)
#undef GO
		default: break;
		}
	}
	cells_launch_general(a, starts);
	VH_CHECK(hipGetLastError());
	return 0;
}

} // namespace vh
