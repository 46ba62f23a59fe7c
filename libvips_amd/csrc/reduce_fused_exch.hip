// The fused RGBA reduce on the matrix cores (reduce_fused_u8.hip) without the tiles' horizontal halo (round 6): what
// BASELINE config 2 runs.  The walks are reduce_fused_step.h's.
//
// reduce_fused_u8x4_mfma reads 512 input columns to make 56 outputs' worth (448): one eighth of its requests are
// columns the tile on either side reads too, and on this part the requests a CU issues bound the stream
// (profiles/NOTES.md 3.1: 2 KB strips without halos stream at 7.1 TB/s, the 59-pixel tiles at 5.8).  Here a tile
// IS 512 aligned columns -- a wave's row segment is four whole 128-byte lines, no column is requested twice -- and
// makes all 64 of its outputs; the six outputs whose 48 taps straddle a tile boundary (three either side) are made
// as PARTIAL SUMS by both tiles, each over its own columns (the T planes carry 48 bytes of zeros either side; at
// the image's edges the edge column, replicated: vips_embed COPY), and a second, tiny kernel adds the two halves
// and rounds them (exact: both are integers below 2^23 in units of 2^-24).  Partial sums and output rows wait in
// LDS and leave in one burst at the tile's end (a trickle of writes would cost the read stream a tenth of its
// rate: tools/write_probe).  Two blocks a CU (78 KB of LDS each), NB row groups in flight per lane, tiles of 128
// output rows: 32 x 16 tiles for BASELINE config 2 = one residency round; requests 1.04 x the image (the
// vertical halo) against 1.22 x.
#include "reduce_fused_step.h"
#include "reduce_u8_host.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

namespace vh {

constexpr int XH = 48;                 // halo bytes either side of a T plane row
constexpr int XPLANE = XH + 512 + XH + 4; // 612 bytes = 153 dwords (odd: 32 planes in 32 banks)
// (the horizontal walk's segment 0 starts 8 * 3 - fx0 <= 48 bytes before a plane row's column 0: inside the halo.  Its
// segment 7 reads up to byte 591 + fx0 <= 575 of the row, past the 48-byte halo into the next plane row -- or, for
// the last plane, the tap tables: harmless, only the discarded outputs 67 / 68 and zero taps (d = 6, 7) read them)
constexpr int XGUARD = 64;             // in front of the planes
constexpr int XPLANES_BYTES = XGUARD + MFMA_SLOTS * 4 * XPLANE;
constexpr int XPART = 48;              // floats per row: [side 2][straddling output 6][channel 4]
constexpr int XMAX_OHT = 128;
static constexpr size_t xlds_bytes(int oht)
{
	return (size_t) XPLANES_BYTES + 2 * MFMA_TABLE_ENTRIES * 8 + (size_t) oht * 64 * 4 + (size_t) oht * XPART * 4;
}

// Profiling builds of the exchange kernel (PROF bits; the shipped kernel is PROF = 0, reduce_exch_prof the others,
// reached only through $VIPS_HIP_FUSED_DEBUG): the load stream alone (no arithmetic, no horizontal pass, no tile end),
// no horizontal pass, no tile end; every row fetched with the default cache policy instead of `nt` (XPROF_L2: what the
// halo rows -- read by both tiles of a row boundary, at about the same time -- can gain from the L2, as a bound)
constexpr int XPROF_LOADS = 1, XPROF_NO_H = 2, XPROF_NO_END = 4, XPROF_L2 = 8;
// ... and the census build (XPROF_CENSUS): the shipped kernel, and thread 0 of every block stamps the chip-wide 100 MHz
// clock at kernel entry, after the prologue's barrier, when the batch loop is done and after the block's last burst
// store has been acknowledged, into a slot of XCENSUS_WORDS 64-bit words behind `parts` (the launcher makes the
// room in this build only, and writes them out: $VIPS_HIP_FUSED_CENSUS, tools/c2_census.py)
constexpr int XPROF_CENSUS = 16;
constexpr int XCENSUS_WORDS = 8; // 4 stamps, XCC id, block index, 2 spare: one 64-byte line a tile

template <int PROF>
__device__ __forceinline__ void census_stamp(unsigned long long *slot, int k, int t)
{
	if constexpr ((PROF & XPROF_CENSUS) != 0) {
		if (t == 0)
			slot[k] = __builtin_amdgcn_s_memrealtime();
	}
}

// LOOP: the K of the explicit wait in front of the steady batches' refills (MfmaStep::throttle).
template <int D, int NB, int PROF, int LOOP>
__device__ __forceinline__ void reduce_fused_x_body(const FusedArgs &a, const MfmaTables *__restrict__ tables,
	float *parts, int *arrivals, int plain, int *misplaced)
{
	constexpr int S = 8;
	typedef MfmaStep<D, !(PROF & XPROF_L2), (PROF & XPROF_LOADS) != 0, XPLANE> Step;
	VH_DYNAMIC_LDS(unsigned char, lds_raw);
	unsigned char *planes = lds_raw + XGUARD + XH; // byte p of a plane row = the tile's own column p
	half4v *lds_a = reinterpret_cast<half4v *>(lds_raw + XPLANES_BYTES);
	half4v *lds_ah = lds_a + MFMA_TABLE_ENTRIES;
	unsigned int *stage = reinterpret_cast<unsigned int *>(lds_ah + MFMA_TABLE_ENTRIES); // oht rows of 64 pixels
	float *part = reinterpret_cast<float *>(stage + a.oht * 64);                           // oht rows of XPART floats

	// XCD k (blocks b = k mod 8) takes WHOLE rows of tiles, a contiguous run of them: horizontal neighbours -- which
	// hand partial sums to each other -- and most vertical ones share an L2
	const int per_xcd = gridDim.x / 8; // = rows of tiles per XCD x tiles_x (host)
	const int tile = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
	if (tile >= a.tiles)
		return;
	const int t = threadIdx.x;
	unsigned long long *census = reinterpret_cast<unsigned long long *>(parts + (size_t) a.tiles * a.oht * XPART) + XCENSUS_WORDS * tile;
	census_stamp<PROF>(census, 0, t);
	const int by = tile / a.tiles_x;
	const int bx = tile - by * a.tiles_x;
	const int y0 = by * a.oht;
	const int oh = min(a.oht, a.out_height - y0);
	const int ca = 512 * bx + 2 * t - a.in_left;
	const bool flip = (by & 1) != 0;
	const int dir = flip ? -1 : 1;
	const int row0 = flip ? a.fy0 + S * (y0 + oh - 1) + S * D - 1 : a.fy0 + S * y0;

	// zeros in the planes (the halos stay zero: a group only ever writes its own 512 columns), the tables
	for (int i = t; i < XPLANES_BYTES / 4; i += FUSED_THREADS)
		reinterpret_cast<unsigned int *>(lds_raw)[i] = 0u;
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
	const bool left_edge = bx == 0, right_edge = bx == a.tiles_x - 1;

	// ---- the horizontal pass over the rows the batch at g0 completed (T row r <-> group g0 + r)
	auto hpass = [&](int g0) __attribute__((always_inline)) {
		const int jlo = max(g0 - (D - 1), 0);
		const int jhi = min(g0 + MFMA_SLOTS - 1 - (D - 1), oh - 1); // inclusive
		if (jhi < jlo)
			return;
		__syncthreads();
		if (left_edge || right_edge) {
			// vips_embed(COPY): the columns beyond the image are its edge column, in every plane row
			for (int i = t; i < MFMA_SLOTS * 4 * (XH / 4); i += FUSED_THREADS) {
				const int rowc = i / (XH / 4), d = i - rowc * (XH / 4);
				unsigned char *prow = planes + rowc * XPLANE;
				if (left_edge)
					*reinterpret_cast<unsigned int *>(prow - XH + 4 * d) = (unsigned int) prow[0] * 0x01010101u;
				if (right_edge)
					*reinterpret_cast<unsigned int *>(prow + 512 + 4 * d) = (unsigned int) prow[511] * 0x01010101u;
			}
			__syncthreads();
		}
		const int nrows = jhi - jlo + 1;
		const int r_lo = jlo - (g0 - (D - 1));
		if (!(PROF & (XPROF_LOADS | XPROF_NO_H))) {
			// thread -> (T row, segment of 9 outputs, channel): segment s makes local outputs 9 s - 3 .. 9 s + 5, the
			// eight of them every output of the tile and the neighbours' three straddling ones either side
			const int hc = t & 3, hr = (t >> 2) & 7, hseg = t >> 5;
			const half4v *lane_ah = lds_ah + hc;
			const bool row_ok = hr < nrows;
			const int lrow = r_lo + (row_ok ? hr : 0);
			const int xs = 9 * hseg - 3; // the segment's first local output
			const unsigned char *line = planes + (lrow * 4 + hc) * XPLANE + a.fx0 + 8 * xs;
			float4v hacc[2];
			hacc[0] = (float4v){ 0.0f, 0.0f, 0.0f, 0.0f };
			hacc[1] = (float4v){ 0.0f, 0.0f, 0.0f, 0.0f };
			unsigned int pix[3] = { 0, 0, 0 };
			float raw[7];
			Step::template hwalk_x<0>(hacc, line, lane_ah, hc, pix, raw);
			if (row_ok) {
				const int jj = jlo + hr;
				unsigned int *srow = stage + jj * 64;
				const int x = xs + 2 * hc; // pix[0], pix[1]: outputs x, x + 1; pix[2] (lane 0): output xs + 8
				if (x >= 0 && x < 64)
					srow[x] = pix[0];
				if (x + 1 >= 0 && x + 1 < 64)
					srow[x + 1] = pix[1];
				if (hc == 0 && xs + 8 < 64)
					srow[xs + 8] = pix[2];
				// straddling outputs, side 0: local outputs -3 .. 2 (segment 0's 0 .. 5), side 1: 61 .. 66 (segment
				// 7's 1 .. 6)
				float *prow = part + jj * XPART + hc;
				if (hseg == 0) {
#pragma unroll
					for (int o = 0; o < 6; o++)
						prow[o * 4] = raw[o];
				}
				else if (hseg == 7) {
#pragma unroll
					for (int o = 0; o < 6; o++)
						prow[24 + o * 4] = raw[1 + o];
				}
			}
		}
		__syncthreads();
	};

	// The row loop.  STEADY batches -- all eight groups there, all eight refills wanted -- run without a branch around
	// a load (MfmaStep::batch_steady: 15 or 16 of a full tile's 17); a tile too short for one, and every tile's last
	// one or two batches, run the guarded form.  The two are loops of their own: where their paths joined inside one
	// loop the compiler would lose count of the loads in flight again and wait for all of them.
	uint2 px[NB][S];
	int g0 = 0;
	if (ngroups >= MFMA_SLOTS + NB) {
		// (a prologue of its own, without the guards: loads behind a branch here and the steady loop's first waits
		// are no longer counted ones)
#pragma unroll
		for (int b = 0; b < NB; b++)
			Step::template load_rows<0, S>(a, px[b], row0 + dir * S * b, dir, ca);
		__syncthreads();
		census_stamp<PROF>(census, 1, t);
		for (; g0 + MFMA_SLOTS + NB <= ngroups; g0 += MFMA_SLOTS) {
			Step::template batch_steady<0, NB, LOOP>(a, px, g0, acc, planes, lane_a, t, row0, dir, ca, 0);
			hpass(g0);
		}
	}
	else {
#pragma unroll
		for (int b = 0; b < NB; b++)
			if (b < ngroups)
				Step::template load_rows<0, S>(a, px[b], row0 + dir * S * b, dir, ca);
		__syncthreads();
		census_stamp<PROF>(census, 1, t);
	}
	for (; g0 < ngroups; g0 += MFMA_SLOTS) {
		Step::template batch<0, NB>(a, px, g0, ngroups, acc, planes, lane_a, t, row0, dir, ca, 0, oh);
		hpass(g0);
	}
	census_stamp<PROF>(census, 2, t);
	if (PROF & (XPROF_LOADS | XPROF_NO_END))
		return;

	// ---- the tile's end.  Its partial sums leave first (write-through); then it ARRIVES at its two boundaries (an
	// atomic counter each: two arrivals a launch, so the parity of what the atomic returns says who is second, launch
	// after launch without a reset).  The LATER tile of a boundary reads the earlier one's halves -- published before
	// that tile arrived -- adds its own, rounds (fin_pack: exact integers below 2^23 in units of 2^-24) and
	// writes all six straddling pixels: its own three through the stage, the neighbour's three straight to the
	// image.  The earlier tile leaves those three alone.  Nobody waits for anybody.  At the image's edges the tile
	// holds the whole sums (the replicated edge column) and is "second" by itself.
	if (a.debug & 32) {
		// ($VIPS_HIP_FUSED_DEBUG=32: the two-kernel form -- partial sums by output row, reduce_fused_edges adds them)
		const int part16 = t & 15;
		for (int r = t >> 4; r < oh; r += 16) {
			unsigned int *dst = reinterpret_cast<unsigned int *>(
				a.out + (long long) (y0 + (flip ? oh - 1 - r : r)) * a.out_stride + (long long) (64 * bx) * 4);
			typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
			*reinterpret_cast<u32x4 *>(dst + 4 * part16) = *reinterpret_cast<const u32x4 *>(stage + r * 64 + 4 * part16);
		}
		float *dstp = parts + (size_t) tile * a.oht * XPART;
		for (int i = t; i < oh * (XPART / 4); i += FUSED_THREADS) {
			const int r = i / (XPART / 4), q = i - r * (XPART / 4);
			const int yrel = flip ? oh - 1 - r : r;
			reinterpret_cast<float4 *>(dstp + (size_t) yrel * XPART)[q] = reinterpret_cast<const float4 *>(part + r * XPART)[q];
		}
		return;
	}
	{
		typedef float f32x4 __attribute__((ext_vector_type(4)));
		const bool placed = VH_XCC_ID() == (int) (blockIdx.x & 7u);
		const bool use_plain = plain && placed;
		if (plain && !placed && t == 0)
			VH_STORE_SYS(misplaced, 1);
		float *dstp = parts + (size_t) tile * a.oht * XPART; // (rows in WALK order: the tiles of a row of tiles share it)
		for (int i = t; i < oh * (XPART / 4); i += FUSED_THREADS) {
			f32x4 *dst = reinterpret_cast<f32x4 *>(dstp) + i;
			const f32x4 v = reinterpret_cast<const f32x4 *>(part)[i];
			// The two tiles of a boundary are neighbours in one row of tiles, and a row of tiles belongs to ONE XCD
			// (the tile numbering above, with block b on XCD b % 8: what the part does, checked by a census launch
			// before `plain` is ever set -- xcc_census_kernel -- and by every block for itself here): their hand-off
			// can stay in that XCD's L2 -- plain stores, read by the other tile with loads that skip ITS L1 --
			// instead of going through to memory (12.6 MB of write-through at the kernel's tail: 0.1914 against
			// 0.1867 ms a launch).  A block that finds itself elsewhere writes through and says so (*misplaced, host
			// memory: the host stops using the plain form and reports it -- never seen).
			if (use_plain)
				*dst = v;
			else
				VH_STORE4_SYS(dst, v);
		}
		VH_WAIT_VMCNT(0);
		__syncthreads();
		int *second = reinterpret_cast<int *>(lds_raw); // (the planes are done with)
		if (t < 2) { // (two lanes: the two atomics travel together)
			int *at = arrivals + by * (a.tiles_x + 1) + bx + t;
			const bool edge = t == 0 ? left_edge : right_edge;
			second[t] = edge ? 1 : (atomicAdd(at, 1) & 1);
		}
		__syncthreads();
		const int sec[2] = { second[0], second[1] };
#pragma unroll 1
		for (int side = 0; side < 2; side++) {
			if (!sec[side])
				continue;
			const bool at_edge = side == 0 ? left_edge : right_edge;
			const float *theirs = parts + (size_t) (tile + (side ? 1 : -1)) * a.oht * XPART + (1 - side) * 24;
			for (int i = t; i < oh * 6; i += FUSED_THREADS) {
				const int r = i / 6, o = i - r * 6;
				const float *mine = part + r * XPART + side * 24 + o * 4;
				float v[4] = { mine[0], mine[1], mine[2], mine[3] };
				if (!at_edge) {
					const float *p = theirs + (size_t) r * XPART + o * 4;
#pragma unroll
					for (int c = 0; c < 4; c++)
						v[c] += VH_LOAD_SYS(p + c);
				}
				unsigned int pxl = fin_pack(v[0], 0, 0);
				pxl = fin_pack(v[1], 1, pxl);
				pxl = fin_pack(v[2], 2, pxl);
				pxl = fin_pack(v[3], 3, pxl);
				const int xl = (side ? 61 : -3) + o; // local output
				if (xl >= 0 && xl < 64)
					stage[r * 64 + xl] = pxl;
				else if (!at_edge)
					*reinterpret_cast<unsigned int *>(a.out + (long long) (y0 + (flip ? oh - 1 - r : r)) * a.out_stride +
						(long long) (64 * bx + xl) * 4) = pxl;
			}
		}
		__syncthreads();
		// the burst: 16 lanes a row, 4 pixels each; the first and the last lane's straddling pixels only if this tile
		// made them
		const int part16 = t & 15;
		for (int r = t >> 4; r < oh; r += 16) {
			unsigned int *dst = reinterpret_cast<unsigned int *>(
				a.out + (long long) (y0 + (flip ? oh - 1 - r : r)) * a.out_stride + (long long) (64 * bx) * 4);
			const unsigned int *src = stage + r * 64 + 4 * part16;
			if ((part16 == 0 && !sec[0]) || (part16 == 15 && !sec[1])) {
				if (part16 == 0)
					dst[3] = src[3];
				else
					dst[60] = src[0];
			}
			else {
				typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
				*reinterpret_cast<u32x4 *>(dst + 4 * part16) = *reinterpret_cast<const u32x4 *>(src);
			}
		}
		if constexpr ((PROF & XPROF_CENSUS) != 0) {
			VH_WAIT_VMCNT(0); // (every wave's stores acknowledged)
			__syncthreads();
			census_stamp<PROF>(census, 3, t);
			if (t == 0) {
				census[4] = (unsigned long long) VH_XCC_ID();
				census[5] = blockIdx.x;
			}
		}
	}
}

// The row loop's steady batches in the shipped kernel and its profiling builds: every quad's refill waits until at most
// 4 of the wave's loads are still in flight (so at most 8 are, of NB * 8 = 32 buffer registers' worth).  Measured
// interleaved (profiles/c2_row_loop.txt, NOTES R8.1): guarded batches 0.1843-0.1850 ms; steady without an explicit wait
// 0.1851, K = 20 / 12 / 8: 0.1858 / 0.1858 / 0.1858, K = 0: 0.2017; K = 4: 0.1797-0.1802.
constexpr int XLOOP = 4;

template <int D, int NB, int OCC>
__global__ void __launch_bounds__(FUSED_THREADS, OCC)
reduce_fused_u8x4_mfma_x(FusedArgs a, const MfmaTables *__restrict__ tables, float *parts, int *arrivals, int plain,
	int *misplaced)
{
	reduce_fused_x_body<D, NB, 0, XLOOP>(a, tables, parts, arrivals, plain, misplaced);
}

template <int D, int NB, int OCC, int PROF>
__global__ void __launch_bounds__(FUSED_THREADS, OCC)
reduce_exch_prof(FusedArgs a, const MfmaTables *__restrict__ tables, float *parts, int *arrivals, int plain,
	int *misplaced)
{
	reduce_fused_x_body<D, NB, PROF, XLOOP>(a, tables, parts, arrivals, plain, misplaced);
}

// The straddling outputs: boundary k (0 .. tiles_x: 0 and tiles_x are the image's edges, where one tile holds the
// whole sum) x output row x the six outputs, one RGBA pixel a thread: the two tiles' halves added (exact) and
// rounded as every other output is (fin_pack).
__global__ void __launch_bounds__(256)
reduce_fused_edges(FusedArgs a, const float *__restrict__ parts)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	const int o = i % 6, k = (i / 6) % (a.tiles_x + 1), y = i / (6 * (a.tiles_x + 1));
	if (y >= a.out_height)
		return;
	const int by = y / a.oht, yrel = y - by * a.oht;
	const int xo = 64 * k - 3 + o;
	if (xo < 0 || xo >= a.out_width)
		return;
	float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	if (k > 0) { // the tile on the left: its side 1
		const float *p = parts + ((size_t) (by * a.tiles_x + k - 1) * a.oht + yrel) * XPART + 24 + o * 4;
		const float4 v = *reinterpret_cast<const float4 *>(p);
		sum = v;
	}
	if (k < a.tiles_x) { // the tile on the right: its side 0
		const float *p = parts + ((size_t) (by * a.tiles_x + k) * a.oht + yrel) * XPART + o * 4;
		const float4 v = *reinterpret_cast<const float4 *>(p);
		sum.x += v.x;
		sum.y += v.y;
		sum.z += v.z;
		sum.w += v.w;
	}
	unsigned int px = fin_pack(sum.x, 0, 0);
	px = fin_pack(sum.y, 1, px);
	px = fin_pack(sum.z, 2, px);
	px = fin_pack(sum.w, 3, px);
	*reinterpret_cast<unsigned int *>(a.out + (long long) y * a.out_stride + (long long) xo * 4) = px;
}

// Does block b of a launch run on XCD b % 8 on this device?  (HIP promises nothing; the part's eight command
// processors each take every eighth workgroup.)  One launch of 2 048 blocks, once per device.
__global__ void xcc_census_kernel(int *wrong)
{
	if (threadIdx.x == 0 && VH_XCC_ID() != (int) (blockIdx.x & 7u))
		atomicAdd(wrong, 1);
}

static bool xcd_placement_holds()
{
	constexpr int MAXDEV = 64;
	static std::mutex mutex;
	static signed char state[MAXDEV];
	const int dev = current_device();
	if (dev < 0 || dev >= MAXDEV)
		return false;
	std::lock_guard<std::mutex> lock(mutex);
	if (state[dev] == 0) {
		state[dev] = -1;
		int zero = 0, wrong = 1;
		int *d = (int *) upload(&zero, sizeof(zero));
		if (d) {
			hipLaunchKernelGGL(xcc_census_kernel, dim3(2048), dim3(64), 0, stream(), d);
			if (hipGetLastError() == hipSuccess && hipMemcpyAsync(&wrong, d, sizeof(wrong), hipMemcpyDeviceToHost, stream()) == hipSuccess &&
				hipStreamSynchronize(stream()) == hipSuccess && wrong == 0)
				state[dev] = 1;
			vips_hip_free(d);
		}
		else
			vips_hip_error_clear();
	}
	return state[dev] == 1;
}

// A kernel of this file may use 80 KB of dynamic LDS: asked for once per device and kernel, not at every launch.
static hipError_t allow_big_lds(const void *kern)
{
	static std::mutex mutex;
	static std::set<std::pair<int, const void *>> done;
	const std::pair<int, const void *> key(current_device(), kern);
	std::lock_guard<std::mutex> lock(mutex);
	if (done.count(key))
		return hipSuccess;
	const hipError_t err = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
	if (err == hipSuccess)
		done.insert(key);
	return err;
}

// The census build's slots, when $VIPS_HIP_FUSED_CENSUS names a file: one line a tile appended to it -- tile, bx, by,
// block index, XCC id, the four stamps in ticks of 10 ns after the launch's earliest.  (Profiling only: it waits for
// the launch.)
static void census_write(const FusedArgs &a, int tiles_y, const void *d_slots)
{
	const char *path = getenv("VIPS_HIP_FUSED_CENSUS");
	if (!path || !*path)
		return;
	std::vector<unsigned long long> slots((size_t) a.tiles * XCENSUS_WORDS);
	if (hipMemcpyAsync(slots.data(), d_slots, slots.size() * sizeof(slots[0]), hipMemcpyDeviceToHost, stream()) != hipSuccess ||
		hipStreamSynchronize(stream()) != hipSuccess) {
		(void) hipGetLastError();
		return;
	}
	unsigned long long first = ~0ull;
	for (int tile = 0; tile < a.tiles; tile++)
		first = slots[(size_t) tile * XCENSUS_WORDS] < first ? slots[(size_t) tile * XCENSUS_WORDS] : first;
	FILE *f = fopen(path, "a");
	if (!f)
		return;
	fprintf(f, "# launch: %d x %d tiles of %d rows; tile bx by block xcc entry prologue loop_done end_done\n", a.tiles_x, tiles_y, a.oht);
	for (int tile = 0; tile < a.tiles; tile++) {
		const unsigned long long *s = &slots[(size_t) tile * XCENSUS_WORDS];
		fprintf(f, "%d %d %d %llu %llu %llu %llu %llu %llu\n", tile, tile % a.tiles_x, tile / a.tiles_x, s[5], s[4], s[0] - first,
			s[1] - first, s[2] - first, s[3] - first);
	}
	fclose(f);
}

// 0 launched, 1 not this kernel's case, -1 error
int launch_fused_mfma_x(const FusedArgs &all, const VipsHipRegion *in, const VipsHipRegion *out,
	const MfmaTables *d_tables)
{
	const char *e = getenv("VIPS_HIP_FUSED_EXCH");
	if (e && atoi(e) == 0)
		return 1;
	if (in->left != 0 || in->width != in->im_width || out->left != 0 || out->width != out->im_width ||
		(in->im_width & 511) || out->width * 8 != in->im_width)
		return 1;
	if (all.fx0 < -(XH - 24) - 0 || all.fx0 > -16 || (all.fx0 & 3) || all.fx0 < -24)
		return 1;
	// (whole 128-byte lines per wave and row are the point of it; forced by the environment -- the parity tests on
	// host fibers, whose "device" memory is malloc's -- 16 bytes do)
	const uintptr_t in_mask = e ? 15 : 127;
	if (((uintptr_t) in->data & in_mask) || (in->stride & in_mask) || ((uintptr_t) out->data & 15) || (out->stride & 15))
		return 1;
	FusedArgs a = all;
	a.tiles_x = in->im_width / 512;
	// one residency round of 2 blocks a CU: as many rows of tiles as 512 slots allow, tiles of 32 .. 128 rows
	int tiles_y = 512 / a.tiles_x;
	const int least = (out->height + XMAX_OHT - 1) / XMAX_OHT;
	tiles_y = tiles_y < least ? least : tiles_y;
	int oht = (out->height + tiles_y - 1) / tiles_y;
	if (oht < 32)
		oht = 32;
	if (oht > XMAX_OHT)
		return 1;
	tiles_y = (out->height + oht - 1) / oht;
	a.oht = oht;
	a.owt = 64;
	a.tiles = a.tiles_x * tiles_y;
	const int want = e ? 1 : 384; // (by default only launches that fill most of the part; $VIPS_HIP_FUSED_EXCH=1: any)
	if (a.tiles < want || a.tiles > 512)
		return 1;
	const int prof = (a.debug >> 6) & 31;
	const size_t parts_bytes = (size_t) a.tiles * a.oht * XPART * sizeof(float);
	const size_t census_bytes = prof == XPROF_CENSUS ? (size_t) a.tiles * XCENSUS_WORDS * sizeof(unsigned long long) : 0;
	const size_t bytes = parts_bytes + census_bytes;
	float *parts = (float *) vips_hip_malloc(bytes);
	if (!parts)
		return -1;
	// the arrival counters: one int per tile boundary, zero once and for the life of the calling thread (a launch
	// adds exactly two to each: see the kernel's end); per thread and device, as the stream the launches are
	// ordered on is
	constexpr int MAX_ARRIVALS = 2048;
	if ((a.tiles_x + 1) * tiles_y > MAX_ARRIVALS) {
		vips_hip_free(parts);
		return 1;
	}
	static thread_local std::map<int, int *> arrivals_by_device;
	int *&arrivals = arrivals_by_device[current_device()];
	if (!arrivals) {
		std::vector<int> zeros(MAX_ARRIVALS, 0);
		arrivals = (int *) upload(zeros.data(), zeros.size() * sizeof(int)); // (kept: a thread's 8 KB)
		if (!arrivals) {
			vips_hip_free(parts);
			return -1;
		}
	}
	// the hand-off through the XCD's L2 (see the kernel): rows of tiles dealt whole to the XCDs, the placement checked
	// once, a word of pinned host memory for a block that finds itself elsewhere.  $VIPS_HIP_FUSED_PLAIN=0: through memory
	static thread_local std::map<int, int *> misplaced_by_device;
	int *&misplaced = misplaced_by_device[current_device()];
	if (!misplaced) {
		misplaced = (int *) vips_hip_malloc_host(64);
		if (misplaced)
			*misplaced = 0;
		else
			vips_hip_error_clear();
	}
	static std::atomic<bool> plain_broken(false);
	if (misplaced && *misplaced) {
		*misplaced = 0;
		if (!plain_broken.exchange(true))
			fprintf(stderr, "vips-hip: reduce: a block ran on another XCD than its index says; the hand-off goes through memory from now on\n");
	}
	const char *pe = getenv("VIPS_HIP_FUSED_PLAIN");
	const int plain = misplaced && !plain_broken.load() && !(pe && atoi(pe) == 0) && xcd_placement_holds() ? 1 : 0;
	const size_t lds = xlds_bytes(a.oht);
	const int rows_per_xcd = (tiles_y + 7) / 8;
	const int grid = 8 * rows_per_xcd * a.tiles_x; // (the kernel's numbering: XCD k takes rows k rows_per_xcd ...)
	// $VIPS_HIP_FUSED_DEBUG bits 64 / 128 / 256: the profiling builds (XPROF_LOADS / NO_H / NO_END; their output is
	// not the image's), 512: XPROF_L2, 1024: XPROF_CENSUS (output unchanged).  (NB = 2 and 1 were measured too, 3-4 %
	// slower than 4: profiles/NOTES.md R7.1)
	typedef void (*XKernel)(FusedArgs, const MfmaTables *, float *, int *, int, int *);
	XKernel kern = reduce_fused_u8x4_mfma_x<6, 4, 2>;
	switch (prof) {
	case XPROF_LOADS: kern = reduce_exch_prof<6, 4, 2, XPROF_LOADS>; break;
	case XPROF_NO_H: kern = reduce_exch_prof<6, 4, 2, XPROF_NO_H>; break;
	case XPROF_NO_END: kern = reduce_exch_prof<6, 4, 2, XPROF_NO_END>; break;
	case XPROF_L2: kern = reduce_exch_prof<6, 4, 2, XPROF_L2>; break;
	case XPROF_CENSUS: kern = reduce_exch_prof<6, 4, 2, XPROF_CENSUS>; break;
	default: break;
	}
	int rc = 0;
	{
		Gate gate("reduce_fused_u8_mfma_x");
		hipError_t err;
		{
			err = allow_big_lds((const void *) kern);
			if (err == hipSuccess)
				hipLaunchKernelGGL(kern, dim3(grid), dim3(FUSED_THREADS), lds, stream(), a, d_tables, parts, arrivals, plain,
					misplaced);
		}
		if (err != hipSuccess || hipGetLastError() != hipSuccess)
			rc = -1;
	}
	if (rc == 0 && (a.debug & 32)) {
		Gate gate("reduce_fused_edges");
		const long long threads = (long long) out->height * (a.tiles_x + 1) * 6;
		hipLaunchKernelGGL(reduce_fused_edges, dim3((unsigned int) ((threads + 255) / 256)), dim3(256), 0, stream(), a, parts);
		if (hipGetLastError() != hipSuccess)
			rc = -1;
	}
	if (rc == 0 && census_bytes && !(a.debug & 32))
		census_write(a, tiles_y, reinterpret_cast<const unsigned char *>(parts) + parts_bytes);
	vips_hip_free(parts); // (the pool hands the block to this thread's LATER work only: ordered on its stream)
	if (rc)
		error("reduce", "kernel launch failed");
	return rc;
}

} // namespace vh
