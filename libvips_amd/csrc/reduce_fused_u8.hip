// uchar fast paths for gfx950 -- see reduce_u8.h.
//
// reduce_fused_u8x4<S, D>: vips_reduce() on uchar RGBA with an even integer
// shrink S on both axes and a constant coefficient phase (input size a
// multiple of S gives phase 0: SURVEY.md appendix "C2 phase arithmetic").
// One launch does reducev (reducev.cpp:418-459) AND reduceh
// (reduceh.cpp:269-328); the vertically reduced scanlines live only in LDS.
//
//   workgroup = 256 threads = one output tile (OWT x OHT pixels)
//   thread t  = input columns col0 + 2t, col0 + 2t + 1 (8 contiguous bytes per
//               row: a wave reads 512 contiguous bytes per scanline)
//   vertical  : the thread walks down the tile's input rows in groups of S.
//               Row S*g + i is tap k = S*d + i of output row g - d, d < D, so D
//               accumulator sets are live and one output row completes per
//               group -- every input byte is loaded from HBM once per tile and
//               used D times from registers.  Rows are paired so one
//               v_dot2_i32_i16 does two taps: v_perm_b32 builds (row r, row r+1)
//               i16 pairs of one channel, the coefficient pair is a scalar.
//   LDS       : a finished row is stored as u16 pairs, planar per channel
//               (plane[row][channel][column]); after R rows a barrier, then
//   horizontal: every thread takes output pixels of the R x OWT strip; its 4
//               channels are D*S/2 dot2 over consecutive LDS dwords
//               (ds_read_b128, 16-byte aligned for S = 8, conflict-free across
//               a wave), rounds, packs RGBA and stores one dword.
//
// Integer arithmetic is exact, so the i32 sums equal the reference's whatever
// the summation order; rounding/clipping is templates.h:152-157.
#include "reduce_fused_step.h"
#include "reduce_u8_host.h"

#include <cstdlib>
#include <vector>

namespace vh {

constexpr int FUSED_SPAN = 2 * FUSED_THREADS; // input columns per tile

// Coefficients travel BY VALUE in the kernel-argument segment: they are read with
// scalar loads (s_load from kernarg memory, dynamic scalar offset), need no device
// allocation and cannot alias the pixel stores.
//   cv / ch = vertical / horizontal i16 coefficient pairs (lo half = even tap).
template <int S, int D>
struct FusedCoefs {
	unsigned int cv[D * (S / 2)];
	unsigned int cv_flip[D * (S / 2)]; // taps reversed, for tiles walked bottom-up
	unsigned int ch[D * (S / 2)];
};

// The accumulator set `slot` holds output row j with j mod D == slot; at input
// group g (rot = g mod D) that row is d = (rot - slot) mod D groups old, i.e. the
// group's rows are its taps S*d .. S*d + S-1.  Accumulators therefore never move:
// the scalar coefficient block rotates instead (one s_load per group).
template <int S, int D>
struct FusedStep {
	static constexpr int PLANE = FUSED_SPAN / 2;
	static constexpr int NP = S * D / 2;
	typedef const unsigned int __attribute__((address_space(4))) *KernargWords;

	// Rows first_row + dir * i, i < S (dir = -1 when the tile is walked bottom-up).
	static __device__ __forceinline__ void load(const FusedArgs &a, uint2 (&px)[S], int first_row,
		int dir, int ca, int cb, bool interior)
	{
		if (interior) {
#pragma unroll
			for (int i = 0; i < S; i++) {
				const int row = min(max(first_row + dir * i, 0), a.im_height - 1) - a.in_top;
				px[i] = *reinterpret_cast<const uint2 *>(a.in + row * a.in_stride + 4 * ca);
			}
		}
		else {
#pragma unroll
			for (int i = 0; i < S; i++) {
				const int row = min(max(first_row + dir * i, 0), a.im_height - 1) - a.in_top;
				const unsigned char *line = a.in + row * a.in_stride;
				px[i].x = *reinterpret_cast<const unsigned int *>(line + 4 * ca);
				px[i].y = *reinterpret_cast<const unsigned int *>(line + 4 * cb);
			}
		}
	}

	// Group ROT (mod D): accumulator set `slot` is d = (ROT - slot) mod D groups old, so
	// this group's rows are its taps S*d .. S*d + S-1.  ROT is a template argument, so the
	// accumulators never move and every coefficient is a kernarg scalar at a fixed offset.
	template <int ROT>
	static __device__ __forceinline__ void accumulate(const uint2 (&px)[S], int (&acc)[D][8],
		KernargWords kcv)
	{
#pragma unroll
		for (int i = 0; i < S; i += 2) {
#pragma unroll
			for (int p = 0; p < 2; p++) {
				const unsigned int ra = p ? px[i].y : px[i].x;
				const unsigned int rb = p ? px[i + 1].y : px[i + 1].x;
#pragma unroll
				for (int c = 0; c < 4; c++) {
					// bytes: [ra.c, 0, rb.c, 0]
					const unsigned int pair =
						__builtin_amdgcn_perm(rb, ra, 0x0c000c00u | (unsigned) c | ((4u + c) << 16));
#pragma unroll
					for (int s = 0; s < D; s++) {
						constexpr int dummy = 0;
						(void) dummy;
						const int d = (ROT - s + D) % D;
						acc[s][p * 4 + c] = dot2(pair, kcv[d * (S / 2) + i / 2], acc[s][p * 4 + c]);
					}
				}
			}
		}
	}

	// Round accumulator set SLOT into LDS row `lds_row` (when it is a real row) and clear it.
	template <int SLOT>
	static __device__ __forceinline__ void retire(int (&acc)[D][8], unsigned int *lds, int lds_row,
		int t, bool store)
	{
		if (store) {
#pragma unroll
			for (int c = 0; c < 4; c++) {
				const unsigned int v = (unsigned) fin_u8(acc[SLOT][c]) |
					((unsigned) fin_u8(acc[SLOT][4 + c]) << 16);
				lds[(lds_row * 4 + c) * PLANE + t] = v;
			}
		}
#pragma unroll
		for (int c = 0; c < 8; c++)
			acc[SLOT][c] = 0;
	}

	// One batch = D consecutive groups (ROT = 0 .. D-1), statically unrolled, with the
	// next group's rows always in flight; group g completes output row g - (D - 1), which
	// lands in LDS row ROT.
	template <int ROT>
	static __device__ __forceinline__ void batch(const FusedArgs &a, uint2 (&cur)[S], uint2 (&nxt)[S],
		int g0, int ngroups, int (&acc)[D][8], unsigned int *lds, KernargWords kcv, int t, int row0,
		int dir, int ca, int cb, bool interior, int oh)
	{
		if constexpr (ROT < D) {
			const int g = g0 + ROT;
			if (g < ngroups) {
				if (g + 1 < ngroups)
					load(a, nxt, row0 + dir * S * (g + 1), dir, ca, cb, interior);
				accumulate<ROT>(cur, acc, kcv);
				const int j = g - (D - 1);
				retire<(ROT + 1) % D>(acc, lds, ROT, t, j >= 0 && j < oh);
			}
			batch<ROT + 1>(a, nxt, cur, g0, ngroups, acc, lds, kcv, t, row0, dir, ca, cb, interior, oh);
		}
	}
};

template <int S, int D>
__global__ void __launch_bounds__(FUSED_THREADS, 4)
reduce_fused_u8x4(FusedArgs a, FusedCoefs<S, D> k_by_value)
{
	// Index the coefficient block where it lies in the kernarg segment (constant
	// address space, scalar loads at immediate offsets).
	typedef FusedStep<S, D> Step;
	typedef typename Step::KernargWords KernargWords;
	static_assert(sizeof(FusedArgs) % alignof(FusedCoefs<S, D>) == 0, "kernarg layout");
	const KernargWords kcv = (KernargWords) ((const char __attribute__((address_space(4))) *)
										   __builtin_amdgcn_kernarg_segment_ptr() +
		sizeof(FusedArgs));
	const KernargWords kch = kcv + 2 * (S * D / 2);
	(void) k_by_value;
	constexpr int NP = S * D / 2; // coefficient pairs
	constexpr int PLANE = FUSED_SPAN / 2; // dwords per (row, channel) plane
	__shared__ __attribute__((aligned(16))) unsigned int lds[D * 4 * PLANE];

	// XCD-aware tile order: block b runs on XCD b % 8, so give every XCD a
	// contiguous run of tiles (row-major): horizontally adjacent tiles share
	// their (D-1)*S-column halo through one L2.
	const int per_xcd = gridDim.x / 8;
	const int tile = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
	if (tile >= a.tiles)
		return;

	const int t = threadIdx.x;
	const int bx = tile % a.tiles_x;
	const int by = tile / a.tiles_x;
	const int x0 = bx * a.owt;
	const int y0 = by * a.oht;
	const int ow = min(a.owt, a.out_width - x0);
	const int oh = min(a.oht, a.out_height - y0);

	// this thread's two input columns, clamped to the image (vips_embed COPY)
	const int tile_col0 = a.fx0 + S * x0;
	const int col0 = tile_col0 + 2 * t;
	const int ca = min(max(col0, 0), a.im_width - 1) - a.in_left;
	const int cb = min(max(col0 + 1, 0), a.im_width - 1) - a.in_left;
	// block-uniform: no column of this tile touches the left/right edge, so every
	// thread reads 8 aligned contiguous bytes per row
	const bool interior = a.aligned8 && tile_col0 >= 0 && tile_col0 + FUSED_SPAN <= a.im_width &&
		(((tile_col0 - a.in_left) & 1) == 0);
	// Serpentine: odd tile rows are walked bottom-up, so a tile reads the (D-1)*S halo
	// rows it shares with its vertical neighbour at the same moment the neighbour does
	// (all tiles are resident and advance in step) and one of the two reads hits L2 /
	// Infinity Cache instead of HBM.  Bottom-up is the same code on the flipped
	// problem: rows counted from the last one, taps reversed (k.cv_flip).
	const bool flip = (by & 1) != 0;
	const int dir = flip ? -1 : 1;
	const int row0 = flip ? a.fy0 + S * (y0 + oh - 1) + S * D - 1 : a.fy0 + S * y0;
	const KernargWords kcv_dir = flip ? kcv + S * D / 2 : kcv;

	int acc[D][8];
#pragma unroll
	for (int d = 0; d < D; d++)
#pragma unroll
		for (int c = 0; c < 8; c++)
			acc[d][c] = 0;

	const int ngroups = oh + D - 1;
	uint2 buf0[S], buf1[S];
	Step::load(a, buf0, row0, dir, ca, cb, interior);

	for (int g0 = 0; g0 < ngroups; g0 += D) {
		Step::template batch<0>(a, buf0, buf1, g0, ngroups, acc, lds, kcv_dir, t, row0, dir, ca, cb, interior, oh);
		if (D & 1) {
			// an odd number of steps leaves the prefetched rows in the other buffer
#pragma unroll
			for (int i = 0; i < S; i++)
				buf0[i] = buf1[i];
		}

		// ---- horizontal pass over the rows this batch completed:
		// j = g0 + r - (D - 1) for r = 0 .. D-1, kept in LDS row r
		const int jlo = max(g0 - (D - 1), 0);
		const int jhi = min(g0, oh - 1); // inclusive
		if (jhi < jlo)
			continue;
		__syncthreads();
		const int nrows = jhi - jlo + 1;
		const int r_lo = jlo - (g0 - (D - 1));
		const int items = nrows * ow;
		for (int it = t; it < items; it += FUSED_THREADS) {
			const int rr = it / ow;
			const int xo = it - rr * ow;
			unsigned int rgba = 0;
#pragma unroll
			for (int c = 0; c < 4; c++) {
				const unsigned int *src = &lds[((r_lo + rr) * 4 + c) * PLANE + xo * (S / 2)];
				int sum = 0;
				if (S % 8 == 0) {
#pragma unroll
					for (int q = 0; q < NP; q += 4) {
						const uint4 v = *reinterpret_cast<const uint4 *>(src + q);
						sum = dot2(v.x, kch[q], sum);
						sum = dot2(v.y, kch[q + 1], sum);
						sum = dot2(v.z, kch[q + 2], sum);
						sum = dot2(v.w, kch[q + 3], sum);
					}
				}
				else if (S % 4 == 0) {
#pragma unroll
					for (int q = 0; q < NP; q += 2) {
						const uint2 v = *reinterpret_cast<const uint2 *>(src + q);
						sum = dot2(v.x, kch[q], sum);
						sum = dot2(v.y, kch[q + 1], sum);
					}
				}
				else {
#pragma unroll
					for (int q = 0; q < NP; q++)
						sum = dot2(src[q], kch[q], sum);
				}
				rgba |= (unsigned) fin_u8(sum) << (8 * c);
			}
			const int jj = jlo + rr; // row of the (possibly flipped) tile
			unsigned int *dst = reinterpret_cast<unsigned int *>(
				a.out + (long long) (y0 + (flip ? oh - 1 - jj : jj)) * a.out_stride);
			dst[x0 + xo] = rgba;
		}
		__syncthreads();
	}
}

// ------------------------------------------------ both passes on the matrix cores
//
// reduce_fused_u8x4_mfma<D> (S = 8): the same tiles and thread <-> column mapping as reduce_fused_u8x4, every tap
// on the MFMA pipe (reduce_u8_device.h; the walks are reduce_fused_step.h's).  The horizontal pass is the same
// computation along x on the u8 T planes in LDS.
//
// Output rows are staged in LDS for the whole tile and written in one burst at its end: on
// this part a 1.5 % stream of writes trickling into a streaming read costs 13 % of the
// read rate (tools/write_probe.hip: 0.175 -> 0.198 ms per GiB), a burst at the end 4 %.
//
// Geometry of a block of 256 threads (four blocks per CU, 59-pixel tiles).  A lane owns two pixels.
// bytes per (row, channel) T plane: 512 samples + 4, so that the 32 planes a half-wave of the
// horizontal pass reads (8 rows x 4 channels, one dword each) fall in 32 distinct banks
constexpr int MFMA_PLANE = FUSED_SPAN + 4; // odd number of dwords: see above
constexpr int MFMA_PLANES_BYTES = MFMA_SLOTS * 4 * MFMA_PLANE;
constexpr int MFMA_STAGE_PITCH = FUSED_SPAN / 8 - 4; // dwords per staged output row (owt <= FUSED_SPAN / 8 - 5)
// (160 KB / blocks per CU) - planes - tables, in staged rows
constexpr int MFMA_MAX_OHT = 88;
// stage_rows = rows the stage must hold: a burst leaves as soon as burst_rows are complete,
// and a horizontal pass completes at most 8 more
static constexpr size_t mfma_lds_bytes(int stage_rows)
{
	return (size_t) MFMA_PLANES_BYTES + 2 * MFMA_TABLE_ENTRIES * 8 + (size_t) stage_rows * MFMA_STAGE_PITCH * 4;
}

// Tiles are numbered row-major and XCD k (blocks b = k mod 8) takes a contiguous range of
// them, so horizontal neighbours (which read their shared halo columns in lock-step) and
// most vertical neighbours (which the serpentine walk makes meet at their shared halo rows)
// share an L2.  Measured on C2: row-major 0.218 ms, column-major 0.221, no serpentine 0.225.
template <int D>
__global__ void __launch_bounds__(FUSED_THREADS, 4)
reduce_fused_u8x4_mfma(FusedArgs a, const MfmaTables *__restrict__ tables)
{
	constexpr int S = 8, NB = 1; // NB: row groups in flight per lane
	typedef MfmaStep<D, true, false, MFMA_PLANE> Step;
	VH_DYNAMIC_LDS(unsigned char, lds_raw);
	// T planes (the horizontal walker over-reads the end of a plane by up to 8 * (D - 1)
	// samples: into the next plane / the tables -- any byte is a finite f16 denormal), the two
	// A-operand tables, the staged output rows of the tile
	unsigned char *planes = lds_raw;
	half4v *lds_a = reinterpret_cast<half4v *>(lds_raw + MFMA_PLANES_BYTES);
	half4v *lds_ah = lds_a + MFMA_TABLE_ENTRIES;
	unsigned int *stage = reinterpret_cast<unsigned int *>(lds_ah + MFMA_TABLE_ENTRIES);

	const int per_xcd = gridDim.x / 8;
	const int tile = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
	if (tile >= a.tiles)
		return;

	const int t = threadIdx.x;
	const int by = tile / a.tiles_x;
	const int bx = tile - by * a.tiles_x;
	const int x0 = bx * a.owt;
	const int y0 = by * a.oht;
	const int ow = min(a.owt, a.out_width - x0);
	const int oh = min(a.oht, a.out_height - y0);

	const int tile_col0 = a.fx0 + S * x0 - a.xshift;
	const int col0 = tile_col0 + 2 * t;
	// Columns clamp to the image (vips_embed COPY) -- and to the window: the window holds every
	// column an output needs (checked by the host), so this only matters to lanes past the
	// tile's last tap, whose reads must stay inside the window too.
	const int lo = max(0, a.in_left), hi = min(a.im_width, a.in_right) - 1;
	// (load_rows) the pair is fetched from columns clamped to [lo, hi - 1]; a lane whose first column is left of lo
	// needs pixel lo twice (y = x), one whose second column is right of hi needs pixel hi twice (x = y)
	const int ca = min(max(col0, lo), hi - 1) - a.in_left;
	const int cb = col0 < lo ? 1 : (col0 + 1 > hi ? 2 : 0);
	const bool flip = (by & 1) != 0;
	const int dir = flip ? -1 : 1;
	const int row0 = flip ? a.fy0 + S * (y0 + oh - 1) + S * D - 1 : a.fy0 + S * y0;

	// the A-operand tables (vertical: this tile's walking direction), 128 entries of 4 halves
	if (t < MFMA_TABLE_ENTRIES) {
		reinterpret_cast<uint2 *>(lds_a)[t] = reinterpret_cast<const uint2 *>(tables->a[flip ? 1 : 0])[t];
		reinterpret_cast<uint2 *>(lds_ah)[t] = reinterpret_cast<const uint2 *>(tables->ah)[t];
	}
	const half4v *lane_a = lds_a + (t & 3);

	float4v acc[8][2];
#pragma unroll
	for (int o = 0; o < 8; o++)
#pragma unroll
		for (int h = 0; h < 2; h++)
			acc[o][h] = (float4v){ 0.0f, 0.0f, 0.0f, 0.0f };

	const int ngroups = oh + D - 1;
	uint2 px[NB][S];
#pragma unroll
	for (int b = 0; b < NB; b++)
		if (b < ngroups)
			Step::template load_rows<0, S>(a, px[b], row0 + dir * S * b, dir, ca);
	__syncthreads();

	// The tile's groups are numbered from `off` instead of 0 (ROT = (g + off) mod 8): the blocks
	// sharing a CU get different offsets, so their horizontal passes -- which issue no loads --
	// and their output bursts fall at different times instead of all at once (every tile of the
	// single residency round starts at the same moment and advances at the same rate).
	const int off = a.stagger ? (((int) blockIdx.x / 256) * a.stagger) & 7 : 0;
	int flushed = 0; // rows of the tile already written out
	for (int v0 = 0; v0 < ngroups + off; v0 += MFMA_SLOTS) {
		const int g0 = v0 - off;
		Step::template batch<0, NB>(a, px, g0, ngroups, acc, planes, lane_a, t, row0, dir, ca, cb, oh);

		// ---- horizontal pass over the rows this batch completed (T row r <-> group g0 + r)
		const int jlo = max(g0 - (D - 1), 0);
		const int jhi = min(g0 + MFMA_SLOTS - 1 - (D - 1), oh - 1); // inclusive
		if (jhi < jlo)
			continue;
		__syncthreads();
		const int nrows = jhi - jlo + 1;
		const int r_lo = jlo - (g0 - (D - 1));
		if (!(a.debug & 1)) {
			// thread -> (T row, segment of HSEG_OUT outputs, channel)
			const int hc = t & 3, hr = (t >> 2) & 7, hseg = t >> 5;
			const half4v *lane_ah = lds_ah + hc;
			const bool row_ok = hr < nrows;
			const int lrow = r_lo + (row_ok ? hr : 0);
			const unsigned char *line = planes + (lrow * 4 + hc) * MFMA_PLANE + 8 * HSEG_OUT * hseg + a.xshift;
			float4v hacc[2];
			hacc[0] = (float4v){ 0.0f, 0.0f, 0.0f, 0.0f };
			hacc[1] = (float4v){ 0.0f, 0.0f, 0.0f, 0.0f };
			unsigned int pix[2] = { 0, 0 };
			Step::template hwalk<0>(hacc, line, lane_ah, hc, pix);
			// lane hc of the quad holds output pixels 2*hc, 2*hc + 1 of the segment
			const int xo = HSEG_OUT * hseg + 2 * hc;
			if (row_ok && xo < MFMA_STAGE_PITCH) {
				const int jj = jlo + hr;
				unsigned int *srow = stage + (jj - flushed) * MFMA_STAGE_PITCH + xo;
				*reinterpret_cast<uint2 *>(srow) = make_uint2(pix[0], pix[1]);
			}
		}
		__syncthreads();

		// ---- output: staged rows leave in bursts of burst_rows (and at the tile's end), a wave
		// per row, a lane per pixel; the next write into the stage is behind the next barrier
		const int done = jhi + 1;
		if ((done - flushed >= a.burst_rows || done == oh) && !(a.debug & 2)) {
			// 16 lanes per row, 4 pixels (one dwordx4 store, dword aligned) per lane: the burst is
			// the kernel's tail, so it wants few, wide store instructions
			constexpr int LPR = FUSED_THREADS / 16; // lanes per row: 4 pixels each
			const int part = t & (LPR - 1);
			for (int r = t / LPR; r < done - flushed; r += 16) {
				const int jj = flushed + r;
				unsigned int *dst = reinterpret_cast<unsigned int *>(
					a.out + (long long) (y0 + (flip ? oh - 1 - jj : jj)) * a.out_stride + (long long) x0 * 4);
				const unsigned int *src = stage + r * MFMA_STAGE_PITCH;
				if (4 * part + 4 <= ow) {
					typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
					typedef u32x4 __attribute__((aligned(4))) u32x4_a4;
					*reinterpret_cast<u32x4_a4 *>(dst + 4 * part) = *reinterpret_cast<const u32x4 *>(src + 4 * part);
				}
				else {
					for (int x = 4 * part; x < ow; x++)
						dst[x] = src[x];
				}
			}
			flushed = done;
		}
		else if (done - flushed >= a.burst_rows || done == oh)
			flushed = done;
	}
}

template <int D>
static int launch_fused_mfma(const FusedArgs &args, int tiles, const MfmaTables *d_tables)
{
	Gate gate("reduce_fused_u8_mfma");
	const int grid = (tiles + 7) / 8 * 8; // XCD remap wants a multiple of 8
	const int stage_rows = args.burst_rows + 7 < args.oht ? args.burst_rows + 7 : args.oht;
	const size_t lds = mfma_lds_bytes(stage_rows);
	hipLaunchKernelGGL(reduce_fused_u8x4_mfma<D>, dim3(grid), dim3(FUSED_THREADS),
		lds, stream(), args, d_tables);
	VH_CHECK(hipGetLastError());
	return 0;
}

template <int S, int D>
static int launch_fused(const FusedArgs &args, int tiles, const std::vector<unsigned int> &pairs_v,
	const std::vector<unsigned int> &pairs_h)
{
	FusedCoefs<S, D> k;
	const int np = D * (S / 2);
	for (int q = 0; q < np; q++) {
		k.cv[q] = pairs_v[q];
		// tap k' of the flipped problem is tap S*D-1-k': reverse the pair order and swap halves
		const unsigned int p = pairs_v[np - 1 - q];
		k.cv_flip[q] = (p >> 16) | (p << 16);
		k.ch[q] = pairs_h[q];
	}
	Gate gate("reduce_fused_u8");
	const int grid = (tiles + 7) / 8 * 8; // XCD remap wants a multiple of 8
	hipLaunchKernelGGL((reduce_fused_u8x4<S, D>), dim3(grid), dim3(FUSED_THREADS), 0, stream(), args, k);
	VH_CHECK(hipGetLastError());
	return 0;
}

} // namespace vh

using namespace vh;

extern "C" {

int vips_hip_reduce_gen_tiled(const VipsHipReduce *reducev, const VipsHipReduce *reduceh,
	const VipsHipRegion *in, const VipsHipRegion *out, int tile)
{
	const char *domain = "reduce";
	if (ensure_init())
		return -1;
	if (!reducev || !reduceh) {
		error(domain, "null reduce");
		return -1;
	}
	if (plan_device(domain, &reducev->device) || plan_device(domain, &reduceh->device))
		return -1;
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (in->format != VIPS_HIP_FORMAT_UCHAR || out->format != VIPS_HIP_FORMAT_UCHAR ||
		(in->bands != 4 && in->bands != F3_BANDS) || out->bands != in->bands)
		return 1;
	const bool three = in->bands == F3_BANDS; // the matrix-core kernel for interleaved bands, or nothing
	if (in->im_height != reducev->in_size || out->im_height != reducev->out_size ||
		in->im_width != reduceh->in_size || out->im_width != reduceh->out_size) {
		error(domain, "region does not belong to an image of the size these reduces were built for");
		return -1;
	}
	if (((uintptr_t) in->data & 3) || (in->stride & 3) ||
		(!three && (((uintptr_t) out->data & 3) || (out->stride & 3))))
		return 1;

	// Geometry: both axes must step by the same even integer with one phase.
	std::vector<ReducePos> pv, ph;
	reduce_positions(reducev, out->top, out->height, tile, pv);
	reduce_positions(reduceh, out->left, out->width, 0, ph);
	int fy0, sy, phase_y, fx0, sx, phase_x;
	if (!positions_regular(pv, &fy0, &sy, &phase_y) || !positions_regular(ph, &fx0, &sx, &phase_x))
		return 1;
	if (out->height == 1)
		sy = sx;
	if (out->width == 1)
		sx = sy;
	if (sx != sy || sx < 2 || (sx & 1))
		return 1;
	const int S = sx;
	const int nv = effective_taps(reducev, phase_y);
	const int nh = effective_taps(reduceh, phase_x);
	const int nmax = nv > nh ? nv : nh;
	const int D = (nmax + S - 1) / S;
	if (!((S == 8 && (D == 6 || D == 7)) || (S == 4 && (D == 6 || D == 7)) ||
			(S == 2 && (D == 6 || D == 7))))
		return 1;
	if (three && (S != 8 || getenv("VIPS_HIP_NO_MFMA") || getenv("VIPS_HIP_NO_FUSED3")))
		return 1;

	// the input window must cover what the two gens need
	int need0, needn;
	vips_hip_reducev_need(reducev, out->top, out->height, &need0, &needn);
	if (need0 < in->top || need0 + needn > in->top + in->height) {
		error(domain, "input region too small: need rows %d..%d", need0, need0 + needn);
		return -1;
	}
	vips_hip_reduceh_need(reduceh, out->left, out->width, &need0, &needn);
	if (need0 < in->left || need0 + needn > in->left + in->width) {
		error(domain, "input region too small: need columns %d..%d", need0, need0 + needn);
		return -1;
	}

	std::vector<unsigned int> pairs_v, pairs_h;
	pack_pairs(reducev, phase_y, S * D, pairs_v);
	pack_pairs(reduceh, phase_x, S * D, pairs_h);

	FusedArgs args;
	args.in = (const unsigned char *) in->data;
	args.in_stride = (long long) in->stride;
	args.in_left = in->left;
	args.in_right = in->left + in->width;
	args.in_top = in->top;
	args.im_width = in->im_width;
	args.im_height = in->im_height;
	args.out = (unsigned char *) out->data;
	args.out_stride = (long long) out->stride;
	args.out_width = out->width;
	args.out_height = out->height;
	args.aligned8 = !(((uintptr_t) in->data & 7) || (in->stride & 7));
	args.small_window = in->stride > 0 && (long long) in->stride * in->height < (1LL << 31);
	{
		const int debug_bits = getenv("VIPS_HIP_FUSED_DEBUG") ? atoi(getenv("VIPS_HIP_FUSED_DEBUG")) : 0;
		args.debug = debug_bits;
	}
	args.fx0 = fx0;
	args.fy0 = fy0;
	args.xshift = 0;
	{
		// the MFMA kernel's whole-pair loads (load_rows) need two columns to clamp a pair to
		const int lo = in->left > 0 ? in->left : 0;
		const int hi1 = in->im_width < in->left + in->width ? in->im_width : in->left + in->width;
		args.pairs = hi1 - lo >= 2;
	}
	args.stagger = 0;
	args.burst_rows = 1 << 20;
	args.owt = FUSED_SPAN / S - D + 1;
	args.tiles_x = (out->width + args.owt - 1) / args.owt;

	_VipsHipReduce *rv = const_cast<_VipsHipReduce *>(reducev);
	// S = 8: both passes on the matrix cores when the exactness bounds hold (mfma_taps)
	if (S == 8 && args.small_window && (args.pairs || three) && !getenv("VIPS_HIP_NO_MFMA")) {
		std::vector<int> taps, taps_h;
		const bool exact_v = mfma_taps(rv, phase_y, D, taps), exact_h = mfma_taps(reduceh, phase_x, D, taps_h);
		if (three && !(exact_v && exact_h))
			return 1;
		if (exact_v && exact_h) {
			const MfmaTables *d_tables =
				mfma_tables_cached(rv, std::make_tuple(-3, phase_y * 128 + phase_x, 8 * D), taps, taps_h, D);
			if (!d_tables)
				return -1;
			if (three)
				return launch_fused_u8x3(D, nh, in, out, fx0, fy0, d_tables);
			// Tile height: ONE residency round (256 CUs x 4 blocks) when the staged rows fit in
			// LDS -- every tile then ends, and bursts its output, at the same time, and
			// neighbouring tiles read their shared halos in lock-step (L2 hits); else the
			// smallest whole number of rounds.
			{
				// Line-aligned tiles: a wave's row segment (64 lanes x 8 bytes) that starts on a
				// 128-byte line costs the memory pipe 4 line requests instead of 5, and on this
				// part the requests a CU can issue, not HBM, bound the stream (tools/hbm_probe2:
				// 2 KB strips at a 1888-byte pitch 5.8 TB/s requested, at a 2048-byte pitch 6.5,
				// 7.1 with nt loads).  So: tile pitch a whole number of lines (owt a multiple
				// of 4 -> 32 * owt bytes), lanes start at the line that holds the first tap.
				// Measured on C2 with whole-pair edge loads: 0.1936 ms aligned (999 tiles of 56
				// columns: more halo), 0.1902 ms with tiles that start at their first tap (1015
				// tiles of 59) -- so alignment is opt-in (VIPS_HIP_FUSED_ALIGN=1).
				// (round 3: with the fix-up at the point of use and nt loads the aligned layout is the
				// faster one on every box measured -- 0.1934 against 0.1979, 0.1920 against 0.1928 --
				// so it is the default where base and stride allow; VIPS_HIP_FUSED_ALIGN=0 for the other)
				const bool align = !(getenv("VIPS_HIP_FUSED_ALIGN") && atoi(getenv("VIPS_HIP_FUSED_ALIGN")) == 0);
				if (align && !(in->stride & 127)) {
					const long long addr = (long long) (uintptr_t) in->data + 4LL * ((long long) fx0 - in->left);
					const int off = (int) (((addr % 128) + 128) % 128); // bytes past a line start
					const int owt = ((FUSED_SPAN - off / 4) / S - D + 1) & ~3;
					if (!(off & 15) && owt >= 32) {
						args.xshift = off / 4;
						args.owt = owt;
					}
				}
				// profiling knob: narrower tiles
				const int owt_env = getenv("VIPS_HIP_FUSED_OWT") ? atoi(getenv("VIPS_HIP_FUSED_OWT")) : 0;
				if (owt_env > 0 && owt_env < args.owt)
					args.owt = owt_env;
				args.tiles_x = (out->width + args.owt - 1) / args.owt;
				const int slots = getenv("VIPS_HIP_FUSED_CAP") ? atoi(getenv("VIPS_HIP_FUSED_CAP")) : 256 * 4;
				const int base = slots / args.tiles_x > 0 ? slots / args.tiles_x : 1;
				int oht = out->height;
				for (int k = 1; k <= 4096; k++) {
					oht = (out->height + base * k - 1) / (base * k);
					if (oht <= MFMA_MAX_OHT)
						break;
				}
				args.oht = oht < 1 ? 1 : oht;
			}
			{
				const char *e = getenv("VIPS_HIP_FUSED_STAGGER");
				args.stagger = e ? atoi(e) & 7 : 0;
				e = getenv("VIPS_HIP_FUSED_BURST");
				const int burst = e ? atoi(e) : 0;
				args.burst_rows = burst > 0 ? (burst + 7) & ~7 : MFMA_MAX_OHT + 8;
			}
			const int tiles_y = (out->height + args.oht - 1) / args.oht;
			const int tiles = args.tiles_x * tiles_y;
			args.tiles = tiles;
			// round 6: whole images whose width is a multiple of 512 -- tiles without a horizontal halo
			// (reduce_fused_u8x4_mfma_x), the straddling outputs by a second small kernel
			if (D == 6) {
				const int r = launch_fused_mfma_x(args, in, out, d_tables);
				if (r <= 0)
					return r;
			}
			if (D == 6)
				return launch_fused_mfma<6>(args, tiles, d_tables);
			if (D == 7)
				return launch_fused_mfma<7>(args, tiles, d_tables);
		}
	}

	if (three)
		return 1;
	// The VALU kernel.  Tile height: tall tiles amortise the (D-1)*S-row vertical halo; short
	// tiles balance the 256 CUs better.  Measured on C2: two residency rounds (256 CUs x
	// 4 resident blocks x 2) is the sweet spot -- 0.249 ms vs 0.259 ms at one round.
	{
		const int capacity = 256 * 8;
		int rows_of_tiles = capacity / args.tiles_x;
		if (rows_of_tiles < 1)
			rows_of_tiles = 1;
		int oht = (out->height + rows_of_tiles - 1) / rows_of_tiles;
		if (oht < 32)
			oht = 32;
		args.oht = oht;
	}
	const int tiles_y = (out->height + args.oht - 1) / args.oht;
	const int tiles = args.tiles_x * tiles_y;
	args.tiles = tiles;

#define FUSED_CASE(SS, DD) \
	if (S == SS && D == DD) \
		return launch_fused<SS, DD>(args, tiles, pairs_v, pairs_h);
	FUSED_CASE(8, 6)
	FUSED_CASE(8, 7)
	FUSED_CASE(4, 6)
	FUSED_CASE(4, 7)
	FUSED_CASE(2, 6)
	FUSED_CASE(2, 7)
#undef FUSED_CASE
	return 1;
}

int vips_hip_reduce_gen(const VipsHipReduce *reducev, const VipsHipReduce *reduceh,
	const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_reduce_gen_tiled(reducev, reduceh, in, out, 0);
}

} // extern "C"
