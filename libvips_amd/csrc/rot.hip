// vips_rot (conversion/rot.c), vips_flip (conversion/flip.c) and the turn + flip pairs of vips_autorot
// (conversion/autorot.c:119-177) on the device (gfx950): exact copies of pels, any band count, any
// non-complex format.
//
// With W x H the input, every operation here is one of
//
//   rows stay rows      out(x, y) = in(FX ? W-1-x : x, FY ? H-1-y : y)          out is W x H
//   columns become rows out(x, y) = in(FX ? W-1-y : y, FY ? H-1-x : x)          out is H x W
//
//   d90 = T|FY   d180 = FX|FY   d270 = T|FX   horizontal = FX   vertical = FY
//   orientation 2 FX, 3 FX|FY, 4 FY (d180 then horizontal), 5 T (d90 then horizontal: the transpose),
//   6 T|FY, 7 T|FX|FY (d270 then horizontal), 8 T|FX
//
// so a turn and the flip behind it are ONE launch: the same kernel walks its output the other way.
//
//   rot_tile<P>    T set.  A 256-thread block owns a tile of TS x TS pels (TS = 64 up to 8-byte pels, 32 for 12 and
//                  16: a tile row is 64 .. 512 bytes).  It reads the tile's row segments with lanes on consecutive
//                  ALIGNED dwords of each segment -- a segment may start and end anywhere (3-band uchar, region
//                  views): the row's byte offset (address & 3) is kept per row, the dwords that lie wholly inside go
//                  as dwords, the one or two that stick out byte by byte -- into LDS at the same offset, so that
//                  global dwords are LDS dwords.  After one barrier the tile's COLUMNS go out as the output's row
//                  segments, again lanes on consecutive aligned dwords of the output, each dword put together from
//                  LDS (one ds_read_b32 when pels are whole dwords, bytes / halves otherwise) and the edges byte-wise.
//                  3-byte pels between rows of whole dwords take a shorter way out: a lane owns 12 bytes = four pels.
//                  LDS pitch: TS * P + 4 bytes = an ODD number of dwords.  A wave's column read walks down the rows:
//                  consecutive lanes are 1 (4-byte pels) .. 4 (1-byte pels) rows apart, and ds_read_b32 / _u8 / _u16
//                  take their bank from (address / 4) mod 32 over 32-lane halves, so with an odd pitch 32 consecutive
//                  rows fall on 32 different banks (4-byte pels and up: conflict-free; 3-byte pels: 32 lanes cover
//                  43 rows, every third bank twice; 1-byte pels: lanes are 4 rows apart, 8 banks, 2-way -- the price of
//                  assembling a dword from four rows).  The 4 spare bytes are room for the row's offset.
//                  Tiles are dealt in 2 x 2 groups, numbered along the input's rows, and XCD k takes a contiguous
//                  range of them (block b runs on XCD b mod 8): the four tiles that share input lines (left / right)
//                  and output lines (above / below) run on one XCD's L2 at about the same time.
//   flip_stream<P> T clear, rows that start on dwords on both sides.  A lane owns 16 bytes (48 for 3-, 6- and
//                  12-byte pels: a whole number of pels and of 16-byte groups) of an output row, loads the mirrored
//                  group with global_load_dwordx4, reverses the pels in registers (v_perm_b32 for pels that are not
//                  whole dwords) and stores with global_store_dwordx4; without FX it is a row-permuted copy.  What
//                  is left of a row (under 16 / 48 bytes) goes through the general kernel.
//   rot_general    one pel a lane, any pel size, all of the above: double images (24- and 32-byte pels), rows the
//                  stream kernel declines, and everything under VIPS_HIP_NO_ROT_TILE / VIPS_HIP_NO_FLIP_STREAM.
#include "gcn.h"
#include "internal.h"
#include "kernel_stmt.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace vh {

constexpr int ROT_THREADS = 256;

constexpr int rot_tile_side_of(int pel) { return pel <= 8 ? 64 : 32; }

struct RotArgs {
	const unsigned char *in;
	unsigned char *out;
	long long in_stride, out_stride; // bytes
	int width, height;               // of the input, pels
	int flipx, flipy;
	int tiles_x, tiles_y, quads_x; // (tile kernel)
	int pel;                       // bytes (general kernel)
	int transpose;                 // (general kernel)
	int chunks;                    // whole 16- / 48-byte groups in a row (stream kernel)
};

// ---------------------------------------------------------------- columns become rows

template <int P, int U>
__global__ void __launch_bounds__(ROT_THREADS)
rot_tile_kernel(RotArgs a)
{
	constexpr int TS = rot_tile_side_of(P);
	constexpr int ROWB = TS * P;
	constexpr int PITCH = ROWB + 4;                       // bytes: an odd number of dwords
	constexpr int SPR = U == 4 ? ROWB / 4 : ROWB / 4 + 1; // aligned dwords a row segment can touch
	__shared__ unsigned int lds32[TS * PITCH / 4];
	unsigned char *lds = (unsigned char *) lds32;

	// block -> tile: XCD k takes a contiguous range of the 2 x 2 groups
	const int per_xcd = (int) gridDim.x / 8;
	const int t = ((int) blockIdx.x % 8) * per_xcd + (int) blockIdx.x / 8;
	const int quad = t >> 2;
	const int tx = 2 * (quad % a.quads_x) + (t & 1);
	const int ty = 2 * (quad / a.quads_x) + ((t >> 1) & 1);
	if (tx >= a.tiles_x || ty >= a.tiles_y)
		return;
	const int x0 = tx * TS, y0 = ty * TS;
	const int tw = min(TS, a.width - x0), th = min(TS, a.height - y0);
	const int tid = (int) threadIdx.x;

	// the tile's rows into LDS: byte q of row r's segment at r * PITCH + (address of the segment & 3) + q
	const unsigned long long in0 = (unsigned long long) a.in + (unsigned long long) y0 * a.in_stride + (unsigned long long) x0 * P;
	const int nbytes = tw * P;
	for (int s = tid; s < th * SPR; s += ROT_THREADS) {
		const int r = s / SPR, d = s - r * SPR;
		const unsigned long long row = in0 + (unsigned long long) r * a.in_stride;
		const int sh = U == 4 ? 0 : (int) (row & 3);
		const gptr_in base = gptr_in_of(row - sh);
		const int q0 = 4 * d - sh;
		if (q0 >= 0 && q0 + 4 <= nbytes)
			lds32[r * (PITCH / 4) + d] = gload32(base, 4 * d);
		else {
#pragma unroll
			for (int k = 0; k < 4; k++)
				if (q0 + k >= 0 && q0 + k < nbytes)
					lds[r * PITCH + 4 * d + k] = gload8(base, 4 * d + k);
		}
	}
	__syncthreads();

	// the tile's columns out: output row (x0 + c, or its mirror) takes th pels, input rows 0 .. th-1 or back
	const int ox0 = a.flipy ? a.height - y0 - th : y0;
	const int obytes = th * P;
	const unsigned int in0_low = (unsigned int) in0, stride_low = (unsigned int) a.in_stride;
	if constexpr (P == 3) {
		// 3-byte pels where both sides' rows are whole dwords and the tile has whole groups of four rows (every
		// tile of an image whose rows are whole dwords, but its last ones): a lane owns 12 bytes of an output row
		// = the pels of four input rows, takes each from the two LDS dwords it lies in, and stores three dwords
		const unsigned long long out0 = (unsigned long long) a.out + (unsigned long long) ox0 * P;
		if (((in0_low | stride_low | (unsigned int) out0 | (unsigned int) a.out_stride) & 3u) == 0 && (th & 3) == 0) {
			for (int s = tid; s < tw * (TS / 4); s += ROT_THREADS) {
				const int c = s / (TS / 4), g = s - c * (TS / 4);
				if (4 * g >= th)
					continue;
				const int oy = a.flipx ? a.width - 1 - (x0 + c) : x0 + c;
				unsigned int pel[4];
#pragma unroll
				for (int i = 0; i < 4; i++) {
					const int j = 4 * g + i;
					const int at = (a.flipy ? th - 1 - j : j) * PITCH + c * P;
					const unsigned long long both = ((unsigned long long) lds32[(at >> 2) + 1] << 32) | lds32[at >> 2];
					pel[i] = (unsigned int) (both >> (8 * (at & 3))) & 0xffffffu;
				}
				const unsigned int w[3] = { pel[0] | (pel[1] << 24), (pel[1] >> 8) | (pel[2] << 16), (pel[2] >> 16) | (pel[3] << 8) };
				gstore_dwords<3>(gptr_out_of(out0 + (unsigned long long) oy * a.out_stride) + 12 * g, w);
			}
			return;
		}
	}
	for (int s = tid; s < tw * SPR; s += ROT_THREADS) {
		const int c = s / SPR, d = s - c * SPR;
		const int oy = a.flipx ? a.width - 1 - (x0 + c) : x0 + c;
		const unsigned long long orow = (unsigned long long) a.out + (unsigned long long) oy * a.out_stride + (unsigned long long) ox0 * P;
		const int sh2 = U == 4 ? 0 : (int) (orow & 3);
		const gptr_out ob = gptr_out_of(orow - sh2) + 4 * d;
		const int q0 = 4 * d - sh2;
		if (q0 + 4 <= 0 || q0 >= obytes)
			continue;
		if constexpr (U == 4) {
			const int j = q0 / P, bb = q0 - j * P;
			const int r = a.flipy ? th - 1 - j : j;
			gstore32(ob, lds32[r * (PITCH / 4) + (c * P + bb) / 4]);
		}
		else {
			unsigned int v = 0;
#pragma unroll
			for (int k = 0; k < 4; k += U) {
				const int q = q0 + k;
				if (q >= 0 && q < obytes) {
					const int j = q / P, bb = q - j * P;
					const int r = a.flipy ? th - 1 - j : j;
					const int at = r * PITCH + (int) ((in0_low + (unsigned int) r * stride_low) & 3u) + c * P + bb;
					if constexpr (U == 2)
						v |= (unsigned int) *(const unsigned short *) (lds + at) << (8 * k);
					else
						v |= (unsigned int) lds[at] << (8 * k);
				}
			}
			if (q0 >= 0 && q0 + 4 <= obytes)
				gstore32(ob, v);
			else {
#pragma unroll
				for (int k = 0; k < 4; k += U)
					if (q0 + k >= 0 && q0 + k < obytes) {
						if constexpr (U == 2)
							gstore16(ob + k, (unsigned short) (v >> (8 * k)));
						else
							gstore8(ob + k, (unsigned char) (v >> (8 * k)));
					}
			}
		}
	}
}

// ---------------------------------------------------------------- rows stay rows

// NB bytes of whole P-byte pels, the pels in the opposite order: one v_perm_b32 per source dword an output dword
// draws on (the selectors are constants once the loops are unrolled; a whole-dword pel is a move)
template <int P, int NB>
VH_DEV void reverse_pels(const unsigned int (&w)[NB / 4], unsigned int (&o)[NB / 4])
{
	constexpr int NP = NB / P;
#pragma unroll
	for (int od = 0; od < NB / 4; od++) {
		unsigned int r = 0;
#pragma unroll
		for (int sd = 0; sd < NB / 4; sd++) {
			unsigned int sel = 0x03020100u; // keep what is there
			bool used = false;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const int j = 4 * od + k;
				const int src = (NP - 1 - j / P) * P + j % P;
				if (src / 4 == sd) {
					sel = (sel & ~(0xffu << (8 * k))) | ((4u + (unsigned int) (src % 4)) << (8 * k));
					used = true;
				}
			}
			if (used)
				r = perm(w[sd], r, sel);
		}
		o[od] = r;
	}
}

constexpr int flip_chunk_of(int pel) { return 16 % pel == 0 ? 16 : 48; }

template <int P>
__global__ void __launch_bounds__(ROT_THREADS)
flip_stream_kernel(RotArgs a)
{
	constexpr int NB = flip_chunk_of(P);
	const int k = (int) blockIdx.x * ROT_THREADS + (int) threadIdx.x;
	if (k >= a.chunks)
		return;
	const unsigned int row_bytes = (unsigned int) a.width * P;
	const unsigned int src = a.flipx ? row_bytes - (unsigned int) (k + 1) * NB : (unsigned int) k * NB;
	for (int y = (int) blockIdx.y; y < a.height; y += (int) gridDim.y) {
		const int iy = a.flipy ? a.height - 1 - y : y;
		const gptr_in ib = gptr_in_of((unsigned long long) a.in + (unsigned long long) iy * a.in_stride);
		const gptr_out ob = gptr_out_of((unsigned long long) a.out + (unsigned long long) y * a.out_stride) + (unsigned int) k * NB;
		unsigned int w[NB / 4], o[NB / 4];
#pragma unroll
		for (int g = 0; g < NB / 16; g++) {
			unsigned int q[4];
			gload128(ib, src + 16 * g, q);
#pragma unroll
			for (int i = 0; i < 4; i++)
				w[4 * g + i] = q[i];
		}
		if (a.flipx)
			reverse_pels<P, NB>(w, o);
		else {
#pragma unroll
			for (int i = 0; i < NB / 4; i++)
				o[i] = w[i];
		}
#pragma unroll
		for (int g = 0; g < NB / 16; g++) {
			const unsigned int q[4] = { o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3] };
			gstore128(ob + 16 * g, q);
		}
	}
}

// ---------------------------------------------------------------- one pel a lane

template <typename UT>
__global__ void __launch_bounds__(ROT_THREADS)
rot_general_kernel(RotArgs a)
{
	const int ow = a.transpose ? a.height : a.width, oh = a.transpose ? a.width : a.height;
	const int ox = (int) blockIdx.x * ROT_THREADS + (int) threadIdx.x;
	if (ox >= ow)
		return;
	const int units = a.pel / (int) sizeof(UT);
	for (int oy = (int) blockIdx.y; oy < oh; oy += (int) gridDim.y) {
		const int u = a.transpose ? oy : ox, v = a.transpose ? ox : oy;
		const int ix = a.flipx ? a.width - 1 - u : u;
		const int iy = a.flipy ? a.height - 1 - v : v;
		const UT *src = (const UT *) (a.in + (long long) iy * a.in_stride + (long long) ix * a.pel);
		UT *dst = (UT *) (a.out + (long long) oy * a.out_stride + (long long) ox * a.pel);
		for (int i = 0; i < units; i++)
			dst[i] = src[i];
	}
}

// ---------------------------------------------------------------- dispatch

constexpr int ROT_GRID_BLOCKS = 256 * 8; // of a launch of the row-preserving kernels

static int rows_grid_of(int blocks_x, int rows)
{
	// enough blocks to fill the part, rows dealt round-robin over grid.y
	int gy = (ROT_GRID_BLOCKS + blocks_x - 1) / blocks_x;
	gy = gy < 1 ? 1 : gy;
	return gy > rows ? rows : gy;
}

// the largest of 8, 4, 2, 1 that divides the pel size and every address a kernel forms
static int common_unit(const RotArgs &a, int most)
{
	const uintptr_t all = (uintptr_t) a.in | (uintptr_t) a.out | (uintptr_t) a.in_stride | (uintptr_t) a.out_stride | (uintptr_t) a.pel;
	int u = most;
	while (u > 1 && all % (uintptr_t) u)
		u >>= 1;
	return u;
}

static void launch_general(const RotArgs &a)
{
	const int ow = a.transpose ? a.height : a.width, oh = a.transpose ? a.width : a.height;
	const int bx = (ow + ROT_THREADS - 1) / ROT_THREADS;
	dim3 grid(bx, rows_grid_of(bx, oh), 1), block(ROT_THREADS, 1, 1);
	Gate gate("rot_general");
	switch (common_unit(a, 8)) {
	case 8: hipLaunchKernelGGL((rot_general_kernel<unsigned long long>), grid, block, 0, stream(), a); break;
	case 4: hipLaunchKernelGGL((rot_general_kernel<unsigned int>), grid, block, 0, stream(), a); break;
	case 2: hipLaunchKernelGGL((rot_general_kernel<unsigned short>), grid, block, 0, stream(), a); break;
	default: hipLaunchKernelGGL((rot_general_kernel<unsigned char>), grid, block, 0, stream(), a); break;
	}
}

template <int P>
static void launch_tile(RotArgs a)
{
	constexpr int TS = rot_tile_side_of(P);
	a.tiles_x = (a.width + TS - 1) / TS;
	a.tiles_y = (a.height + TS - 1) / TS;
	a.quads_x = (a.tiles_x + 1) / 2;
	const long long quads = (long long) a.quads_x * ((a.tiles_y + 1) / 2);
	const int blocks = (int) ((quads * 4 + 7) / 8 * 8); // the XCD deal wants a multiple of 8
	dim3 grid(blocks, 1, 1), block(ROT_THREADS, 1, 1);
	char name[32];
	snprintf(name, sizeof(name), "rot_tile<%d>", P);
	Gate gate(name);
	const int unit = common_unit(a, 4);
	if constexpr (P % 4 == 0) {
		if (unit == 4) {
			hipLaunchKernelGGL((rot_tile_kernel<P, 4>), grid, block, 0, stream(), a);
			return;
		}
	}
	if constexpr (P % 2 == 0) {
		if (unit >= 2) {
			hipLaunchKernelGGL((rot_tile_kernel<P, 2>), grid, block, 0, stream(), a);
			return;
		}
	}
	hipLaunchKernelGGL((rot_tile_kernel<P, 1>), grid, block, 0, stream(), a);
}

template <int P>
static void launch_stream(RotArgs a)
{
	constexpr int NB = flip_chunk_of(P);
	const int bx = (a.chunks + ROT_THREADS - 1) / ROT_THREADS;
	dim3 grid(bx, rows_grid_of(bx, a.height), 1), block(ROT_THREADS, 1, 1);
	{
		Gate gate("flip_stream");
		hipLaunchKernelGGL((flip_stream_kernel<P>), grid, block, 0, stream(), a);
	}
	// the ragged end of every row: the output's last pels, which with FX are the input's first
	const int done = a.chunks * (NB / P);
	if (done < a.width) {
		RotArgs e = a;
		e.out += (size_t) done * P;
		if (!a.flipx)
			e.in += (size_t) done * P;
		e.width = a.width - done;
		launch_general(e);
	}
}

static bool stream_ok(const RotArgs &a)
{
	if (getenv("VIPS_HIP_NO_FLIP_STREAM"))
		return false;
	const uintptr_t all = (uintptr_t) a.in | (uintptr_t) a.out | (uintptr_t) a.in_stride | (uintptr_t) a.out_stride;
	if (all % 4 || flip_chunk_of(a.pel) % a.pel)
		return false;
	// the mirrored group starts (width * pel - a multiple of 16) bytes into the row
	if (a.flipx && ((size_t) a.width * a.pel) % 4)
		return false;
	return (size_t) a.width * a.pel >= (size_t) flip_chunk_of(a.pel) && (long long) a.width * a.pel < (1LL << 31);
}

int orientation_op(int orientation)
{
	static const int ops[9] = { 0, 0, ROT_OP_FLIPX, ROT_OP_FLIPX | ROT_OP_FLIPY, ROT_OP_FLIPY, ROT_OP_TRANSPOSE,
		ROT_OP_TRANSPOSE | ROT_OP_FLIPY, ROT_OP_TRANSPOSE | ROT_OP_FLIPX | ROT_OP_FLIPY, ROT_OP_TRANSPOSE | ROT_OP_FLIPX };
	return orientation >= 0 && orientation <= 8 ? ops[orientation] : 0;
}

int rot_op_gen(const char *domain, int op, const VipsHipRegion *in, const VipsHipRegion *out)
{
	if (ensure_init())
		return -1;
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (in->bands != out->bands || in->format != out->format) {
		error(domain, "input and output must have the same bands and format");
		return -1;
	}
	const bool transpose = (op & ROT_OP_TRANSPOSE) != 0;
	if (out->width != (transpose ? in->height : in->width) || out->height != (transpose ? in->width : in->height)) {
		error(domain, "output region must be %d x %d", transpose ? in->height : in->width,
			transpose ? in->width : in->height);
		return -1;
	}
	if (in->data == out->data) {
		error(domain, "cannot work in place");
		return -1;
	}
	RotArgs a = {};
	a.in = (const unsigned char *) in->data;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) out->stride;
	a.width = in->width;
	a.height = in->height;
	a.flipx = (op & ROT_OP_FLIPX) != 0;
	a.flipy = (op & ROT_OP_FLIPY) != 0;
	a.transpose = transpose;
	a.pel = region_elems_per_pel(in) * format_sizeof(format_real(in->format));
	if ((long long) a.width * a.pel >= (1LL << 31) || (long long) a.height * a.pel >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	if (transpose && !getenv("VIPS_HIP_NO_ROT_TILE")) {
		switch (a.pel) {
#define GO(P) \
	case P: \
		launch_tile<P>(a); \
		VH_CHECK(hipGetLastError()); \
		return 0;
			GO(1) GO(2) GO(3) GO(4) GO(6) GO(8) GO(12) GO(16)
#undef GO
		default: break;
		}
	}
	if (!transpose && !a.flipx) { // a row-permuted copy does not care what a pel is: rows of bytes
		a.width *= a.pel;
		a.pel = 1;
	}
	if (!transpose && stream_ok(a)) {
		a.chunks = (int) ((size_t) a.width * a.pel / flip_chunk_of(a.pel));
		switch (a.pel) {
#define GO(P) \
	case P: \
		launch_stream<P>(a); \
		VH_CHECK(hipGetLastError()); \
		return 0;
			GO(1) GO(2) GO(3) GO(4) GO(6) GO(8) GO(12) GO(16)
#undef GO
		default: break;
		}
	}
	launch_general(a);
	VH_CHECK(hipGetLastError());
	return 0;
}

} // namespace vh

extern "C" {

int vips_hip_rot_gen(int angle, const VipsHipRegion *in, const VipsHipRegion *out)
{
	static const int ops[4] = { 0, vh::ROT_OP_TRANSPOSE | vh::ROT_OP_FLIPY, vh::ROT_OP_FLIPX | vh::ROT_OP_FLIPY, vh::ROT_OP_TRANSPOSE | vh::ROT_OP_FLIPX };
	if (angle < 0 || angle > 3) {
		vh::error("rot", "bad angle %d", angle);
		return -1;
	}
	return vh::rot_op_gen("rot", ops[angle], in, out);
}

int vips_hip_flip_gen(int direction, const VipsHipRegion *in, const VipsHipRegion *out)
{
	if (direction != 0 && direction != 1) {
		vh::error("flip", "bad direction %d", direction);
		return -1;
	}
	return vh::rot_op_gen("flip", direction == 0 ? vh::ROT_OP_FLIPX : vh::ROT_OP_FLIPY, in, out);
}

int vips_hip_rot_tile_side(int pel_size)
{
	switch (pel_size) {
	case 1: case 2: case 3: case 4: case 6: case 8: case 12: case 16:
		return vh::rot_tile_side_of(pel_size);
	default:
		return 0;
	}
}

int vips_hip_rot_step(int what)
{
	switch (what) {
	case 0: return vh::ROT_THREADS;
	case 1: return vh::ROT_GRID_BLOCKS;
	default: return 0;
	}
}

int vips_hip_rot_group(int pel_size)
{
	switch (pel_size) {
	case 1: case 2: case 3: case 4: case 6: case 8: case 12: case 16:
		return vh::flip_chunk_of(pel_size);
	default:
		return 0;
	}
}

} // extern "C"
