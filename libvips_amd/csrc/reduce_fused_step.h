// The vertical walk and the horizontal walks of the fused RGBA reduce on the matrix cores, shared by the kernel whose
// tiles have halos (reduce_fused_u8.hip) and the one whose tiles exchange partial sums (reduce_fused_exch.hip), and
// the argument block both take.  The arithmetic is reduce_u8_device.h's.
#pragma once

#include "reduce_u8_device.h"

namespace vh {

struct FusedArgs {
	const unsigned char *in;
	long long in_stride;
	int in_left, in_top;   // origin of the input window
	int in_right;          // in_left + window width
	int pairs;             // MFMA kernel: every tile can fetch whole pixel pairs (see load_rows)
	int stagger;           // MFMA kernel: groups of phase shift between the 4 blocks of a CU
	int burst_rows;        // MFMA kernel: staged output rows per burst (a multiple of 8)
	int im_width, im_height;
	unsigned char *out;
	long long out_stride;
	int out_width, out_height; // region being generated
	int fx0, fy0;              // first tap (un-embedded input coords) of output (0, 0) of the region
	int owt, oht;              // tile size in output pixels
	int tiles_x, tiles;
	int aligned8;           // input base and stride are multiples of 8 bytes
	int small_window;       // the input window spans < 2 GB: 32-bit byte offsets are safe
	int debug;              // VIPS_HIP_FUSED_DEBUG ablation bits (profiling only; 0 in production)
	int xshift;             // MFMA kernel: a tile's lanes start this many columns left of its first tap,
	                        // so that every wave's 512-byte row segment starts on a 128-byte line
};

// NT: streaming (nt) loads; LOADS_ONLY: the profiling build that consumes the rows without arithmetic; PLANE: bytes
// per (row, channel) T plane.  (Rounds 2-5 kept more forms -- the edge fix-up at the loads, two dword loads per lane
// and row, 512 threads, an arithmetic-only build; their measurements are in profiles/NOTES.md 3.1.)
template <int D, bool NT, bool LOADS_ONLY, int PLANE>
struct MfmaStep {
	static constexpr int S = 8;
	// quad()'s refill: guarded by `more` (REFILL_GUARDED), or unconditional -- a steady batch, batch_steady() -- behind
	// an explicit wait that caps the wave at K + 4 loads in flight.  (VH_WAIT_VMCNT spells its argument into the
	// instruction, so K is a literal here: 4, what the exchange kernel ships with.  The other values measured on it --
	// no explicit wait, 0, 8, 12, 20 -- are in profiles/c2_row_loop.txt; an arm a value brings them back.)
	static constexpr int REFILL_GUARDED = -2;

	template <int K>
	static __device__ __forceinline__ void throttle()
	{
		static_assert(K == REFILL_GUARDED || K == 4, "a literal the macro can spell");
		if constexpr (K == 4)
			VH_WAIT_VMCNT(4);
	}

	// Rows first_row + dir * i, I0 <= i < I0 + N.  The launcher only picks these kernels for
	// windows < 2 GB, so every address is the uniform base (an SGPR pair) plus one 32-bit lane
	// offset: the saddr form of global_load, no 64-bit VALU address arithmetic.  Every lane
	// fetches its two pixels as one dwordx2 from the clamped PAIR at column ca (dword alignment
	// is all a dwordx2 load needs); lanes of an edge tile that lie wholly outside the image
	// duplicate the edge pixel where the rows are consumed (quad(): cb = 1: y = x, left;
	// cb = 2: x = y, right).
	template <int I0, int N>
	static __device__ __forceinline__ void load_rows(const FusedArgs &a, uint2 (&px)[S], int first_row,
		int dir, int ca)
	{
		const unsigned int stride32 = (unsigned int) a.in_stride;
#pragma unroll
		for (int i = I0; i < I0 + N; i++) {
			const int row = min(max(first_row + dir * i, 0), a.im_height - 1) - a.in_top;
			const unsigned int off = (unsigned int) row * stride32 + (unsigned int) (4 * ca);
			typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
			const u32x2 *src = reinterpret_cast<const u32x2 *>(a.in + (size_t) off);
			const u32x2 v = NT ? __builtin_nontemporal_load(src) : *src;
			px[i] = make_uint2(v.x, v.y);
		}
	}

	// One quad (rows 4*Q .. 4*Q+3 of the group) of both pixels; once its B operands exist the
	// quad's buffer registers are refilled with the rows of group g + NB.
	template <int ROT, int Q, int K = REFILL_GUARDED>
	static __device__ __forceinline__ void quad(const FusedArgs &a, uint2 (&px)[S], float4v (&acc)[8][2],
		const half4v *lane_a /* &table[lane & 3] */, bool more, int next_row, int dir, int ca, int cb)
	{
		if constexpr (LOADS_ONLY) { // profiling: consume the rows, refill, no arithmetic
#pragma unroll
			for (int i = 4 * Q; i < 4 * Q + 4; i++)
				VH_USE2(px[i].x, px[i].y);
			throttle<K>();
			if (K != REFILL_GUARDED || more)
				load_rows<4 * Q, 4>(a, px, next_row, dir, ca);
			return;
		}
		const half4v a0 = lane_a[((ROT * 2 + Q) * 2 + 0) * 4];
		const half4v a1 = lane_a[((ROT * 2 + Q) * 2 + 1) * 4];
		uint2 row[4];
#pragma unroll
		for (int i = 0; i < 4; i++) {
			row[i] = px[4 * Q + i];
			// the edge fix-up, at the point of use: applied at the loads it made every wave wait for the loads it
			// had just issued, so a wave's own matrix work never ran under its own loads (branch-free: all other
			// lanes carry cb = 0, the compares live in SGPR masks)
			const unsigned int x = row[i].x, y = row[i].y;
			row[i].y = cb == 1 ? x : y;
			row[i].x = cb == 2 ? y : x;
		}
#pragma unroll
		for (int p = 0; p < 2; p++) {
			const unsigned int r0 = p ? row[0].y : row[0].x;
			const unsigned int r1 = p ? row[1].y : row[1].x;
			const unsigned int r2 = p ? row[2].y : row[2].x;
			const unsigned int r3 = p ? row[3].y : row[3].x;
			half4v b[4];
			b[0] = make_b<0>(r0, r1, r2, r3);
			b[1] = make_b<1>(r0, r1, r2, r3);
			b[2] = make_b<2>(r0, r1, r2, r3);
			b[3] = make_b<3>(r0, r1, r2, r3);
			if (p == 1) {
				throttle<K>();
				if (K != REFILL_GUARDED || more)
					load_rows<4 * Q, 4>(a, px, next_row, dir, ca);
			}
#pragma unroll
			for (int c = 0; c < 4; c++) {
				acc[p * 4 + c][0] = __builtin_amdgcn_mfma_f32_4x4x4f16(a0, b[c], acc[p * 4 + c][0], 0, 0, 0);
				acc[p * 4 + c][1] = __builtin_amdgcn_mfma_f32_4x4x4f16(a1, b[c], acc[p * 4 + c][1], 0, 0, 0);
			}
		}
	}

	// Slot (ROT - (D - 1)) mod 8 has seen all its taps: round it into T row `lds_row`.
	template <int ROT>
	static __device__ __forceinline__ void retire(float4v (&acc)[8][2], unsigned char *planes, int lds_row,
		int t, bool store)
	{
		constexpr int SLOT = (ROT - (D - 1) + 2 * MFMA_SLOTS) % MFMA_SLOTS;
		constexpr int H = SLOT >> 2, I = SLOT & 3;
		if (store) {
#pragma unroll
			for (int c = 0; c < 4; c++) {
				const unsigned int v = fin_pack(acc[4 + c][H][I], 1, fin_pack(acc[c][H][I], 0, 0));
				*reinterpret_cast<unsigned short *>(planes + (lds_row * 4 + c) * PLANE + 2 * t) =
					(unsigned short) v;
			}
		}
#pragma unroll
		for (int o = 0; o < 8; o++)
			acc[o][H][I] = 0.0f;
	}

	// The horizontal pass is the same computation along x: a lane owns one (row, channel)
	// line segment of the T planes and walks it in groups of 8 samples; sample group G
	// is d = (G - s) mod 8 groups into output xo = first + s, one output retires per group.
	// The four channel lanes of a quad OR their bytes together (two quad_perm DPP moves)
	// and lane O / 2 keeps the RGBA pixel of output O.
	template <int G>
	static __device__ __forceinline__ void hwalk(float4v (&hacc)[2], const unsigned char *line,
		const half4v *lane_ah, int hc, unsigned int (&pix)[2])
	{
		constexpr int NG = HSEG_OUT + D - 1;
		if constexpr (G < NG) {
			constexpr int ROT = G % MFMA_SLOTS;
			const half4v b0 = bytes_b(*reinterpret_cast<const unsigned int *>(line + 8 * G));
			const half4v b1 = bytes_b(*reinterpret_cast<const unsigned int *>(line + 8 * G + 4));
			hacc[0] = __builtin_amdgcn_mfma_f32_4x4x4f16(lane_ah[((ROT * 2 + 0) * 2 + 0) * 4], b0, hacc[0], 0, 0, 0);
			hacc[1] = __builtin_amdgcn_mfma_f32_4x4x4f16(lane_ah[((ROT * 2 + 0) * 2 + 1) * 4], b0, hacc[1], 0, 0, 0);
			hacc[0] = __builtin_amdgcn_mfma_f32_4x4x4f16(lane_ah[((ROT * 2 + 1) * 2 + 0) * 4], b1, hacc[0], 0, 0, 0);
			hacc[1] = __builtin_amdgcn_mfma_f32_4x4x4f16(lane_ah[((ROT * 2 + 1) * 2 + 1) * 4], b1, hacc[1], 0, 0, 0);
			constexpr int SLOT = (ROT - (D - 1) + 2 * MFMA_SLOTS) % MFMA_SLOTS;
			constexpr int H = SLOT >> 2, I = SLOT & 3;
			if constexpr (G >= D - 1) {
				constexpr int O = G - (D - 1);
				int v = (int) fin_pack(hacc[H][I], (unsigned int) hc, 0);
				v |= __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true); // quad_perm [1,0,3,2]
				v |= __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true); // quad_perm [2,3,0,1]
				if (hc == O / 2)
					pix[O & 1] = (unsigned int) v;
			}
			hacc[H][I] = 0.0f;
			if constexpr ((G & 1) == 1)
				__builtin_amdgcn_sched_barrier(0); // keep the unrolled walk's LDS reads from piling up
			hwalk<G + 1>(hacc, line, lane_ah, hc, pix);
		}
	}

	// The exchange kernel's walk: a segment of 9 outputs (eight segments cover the tile's 64 outputs and
	// the three either side that straddle its boundaries, -3 .. 68, in ONE pass of the whole block).  Output O of
	// the segment uses slot O mod 8 from group O on: output 8 takes slot 0 after output 0 has retired, the table's
	// zero taps (d = 6, 7) keep the slot clear in between.  Lane hc keeps outputs 2 hc, 2 hc + 1 (pix[0], pix[1]),
	// lane 0 output 8 as well (pix[2]); every lane hands out the UNROUNDED sums of its channel's outputs 0 .. 6
	// (raw): the partial sums of the straddling outputs.
	template <int G>
	static __device__ __forceinline__ void hwalk_x(float4v (&hacc)[2], const unsigned char *line, const half4v *lane_ah,
		int hc, unsigned int (&pix)[3], float (&raw)[7])
	{
		constexpr int NG = 9 + D - 1;
		if constexpr (G < NG) {
			constexpr int ROT = G % MFMA_SLOTS;
			const half4v b0 = bytes_b(*reinterpret_cast<const unsigned int *>(line + 8 * G));
			const half4v b1 = bytes_b(*reinterpret_cast<const unsigned int *>(line + 8 * G + 4));
			hacc[0] = __builtin_amdgcn_mfma_f32_4x4x4f16(lane_ah[((ROT * 2 + 0) * 2 + 0) * 4], b0, hacc[0], 0, 0, 0);
			hacc[1] = __builtin_amdgcn_mfma_f32_4x4x4f16(lane_ah[((ROT * 2 + 0) * 2 + 1) * 4], b0, hacc[1], 0, 0, 0);
			hacc[0] = __builtin_amdgcn_mfma_f32_4x4x4f16(lane_ah[((ROT * 2 + 1) * 2 + 0) * 4], b1, hacc[0], 0, 0, 0);
			hacc[1] = __builtin_amdgcn_mfma_f32_4x4x4f16(lane_ah[((ROT * 2 + 1) * 2 + 1) * 4], b1, hacc[1], 0, 0, 0);
			constexpr int SLOT = (ROT - (D - 1) + 2 * MFMA_SLOTS) % MFMA_SLOTS;
			constexpr int H = SLOT >> 2, I = SLOT & 3;
			if constexpr (G >= D - 1) {
				constexpr int O = G - (D - 1);
				if constexpr (O < 7)
					raw[O] = hacc[H][I];
				int v = (int) fin_pack(hacc[H][I], (unsigned int) hc, 0);
				v |= __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true); // quad_perm [1,0,3,2]
				v |= __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true); // quad_perm [2,3,0,1]
				if (hc == (O / 2 & 3))
					pix[O / 2 == 4 ? 2 : O & 1] = (unsigned int) v;
			}
			hacc[H][I] = 0.0f;
			if constexpr ((G & 1) == 1)
				__builtin_amdgcn_sched_barrier(0);
			hwalk_x<G + 1>(hacc, line, lane_ah, hc, pix, raw);
		}
	}

	// NB = prefetch depth: group g lives in ring buffer g mod NB (NB divides 8, so the index is
	// static) and each of its quads is refilled with group g + NB as soon as it has been consumed.
	template <int ROT, int NB>
	static __device__ __forceinline__ void batch(const FusedArgs &a, uint2 (&px)[NB][S], int g0, int ngroups,
		float4v (&acc)[8][2], unsigned char *planes, const half4v *lane_a, int t, int row0, int dir, int ca,
		int cb, int oh)
	{
		if constexpr (ROT < MFMA_SLOTS) {
			const int g = g0 + ROT;
			if (g >= 0 && g < ngroups) {
				// (the guarded form: the compiler cannot count loads across the joins of these branches and waits
				// for ALL of a wave's loads twice a batch -- vmcnt(0) inside group 0 and in front of group 4.
				// The halo kernel runs nothing else: there, at 16 waves a CU and one group in flight per lane,
				// the branch-free form with exact waits was slower, 0.1977 against 0.1932 ms, round 3.  The
				// exchange kernel -- 8 waves a CU, NB = 4 -- runs only its head and rest this way; its steady
				// batches are batch_steady(), measured on that kernel: profiles/c2_row_loop.txt, NOTES R8.1)
				const bool more = g + NB < ngroups;
				const int next_row = row0 + dir * S * (g + NB);
				quad<ROT, 0>(a, px[ROT % NB], acc, lane_a, more, next_row, dir, ca, cb);
				quad<ROT, 1>(a, px[ROT % NB], acc, lane_a, more, next_row, dir, ca, cb);
				const int j = g - (D - 1);
				retire<ROT>(acc, planes, ROT, t, j >= 0 && j < oh);
			}
			batch<ROT + 1, NB>(a, px, g0, ngroups, acc, planes, lane_a, t, row0, dir, ca, cb, oh);
		}
	}

	// A STEADY batch: all eight groups exist and all eight refills are wanted (g0 + MFMA_SLOTS + NB <= ngroups, the
	// caller's to know), so no branch stands around a load or around the consumption of loaded rows and the
	// compiler's waits are counted ones -- vmcnt(30) / vmcnt(28) in front of a group's two quads: a quad is consumed
	// with the 28 newer loads still in flight, unless K says otherwise.  Only the first batch of a tile has slots
	// that retire nothing (j < 0); that predicate is around LDS stores alone.  What this measured on the exchange
	// kernel (0.1843-0.1850 ms guarded): everything up to the tile's end 6.5 us shorter without a wait and with
	// K = 20, 12 and 4, but the whole kernel only with K = 4 (0.1797-0.1802 ms; no wait 0.1851, K = 20 / 12 / 8
	// 0.1858, K = 0 0.2017): with more than eight loads a wave in flight the launch's end gives the gain back.
	template <int ROT, int NB, int K>
	static __device__ __forceinline__ void batch_steady(const FusedArgs &a, uint2 (&px)[NB][S], int g0,
		float4v (&acc)[8][2], unsigned char *planes, const half4v *lane_a, int t, int row0, int dir, int ca, int cb)
	{
		static_assert(K != REFILL_GUARDED, "a steady batch refills unconditionally");
		if constexpr (ROT < MFMA_SLOTS) {
			const int next_row = row0 + dir * S * (g0 + ROT + NB);
			quad<ROT, 0, K>(a, px[ROT % NB], acc, lane_a, true, next_row, dir, ca, cb);
			quad<ROT, 1, K>(a, px[ROT % NB], acc, lane_a, true, next_row, dir, ca, cb);
			retire<ROT>(acc, planes, ROT, t, ROT >= D - 1 || g0 > 0);
			batch_steady<ROT + 1, NB, K>(a, px, g0, acc, planes, lane_a, t, row0, dir, ca, cb);
		}
	}
};

} // namespace vh
