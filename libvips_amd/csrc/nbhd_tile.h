// The halo tile of the neighbourhood filters (rank.hip, morph.hip, edge.hip, hist_local.hip): what a block stages in LDS
// before it filters.
//
// A block makes TW elements x TH rows of the output.  Output element e (an element is one band of one pel) of row y
// reads the input elements e + (i - win_w / 2) * bands, i = 0 .. win_w - 1, of rows y + j - win_h / 2, j = 0 ..
// win_h - 1, with the PEL coordinates clamped to the image: the vips_embed(VIPS_EXTEND_COPY) the reference puts in
// front (morphology/rank.c:507-511, morph.c:858-863).  The block's LDS holds TH + win_h - 1 rows of `lds_row` bytes;
// byte 0 of a row is image element `e_start` of that row: the tile's first element less the left halo, rounded DOWN
// to a whole dword so that, on images whose rows start on dwords, every 16-byte group of an LDS row is 16 bytes of
// the image row at a 4-byte aligned address.  A group takes one of three ways in:
//   - wholly inside the input window at an aligned address: one global_load_dwordx4;
//   - wholly inside, not aligned (rows of a uchar image whose stride is no multiple of 4): element loads;
//   - across an edge of the image or of the window: element loads with the pel clamped, first to the image -- the
//     edge copy -- then to the window (for the padding elements nobody reads: nothing outside the window is touched).
// Elements are stored as KEYS: `key_xor` is XORed on every dword (the sign bits of a signed format, so that unsigned
// order is the format's order; all ones on top to turn a maximum into a minimum; 0 for morph), and float keys are
// the usual sign flip.  The callers turn a key back with nb_unkey().
// nb_stage<.., MIRROR = true> reflects at the image's edges instead of copying them: vips_embed(VIPS_EXTEND_MIRROR), which
// vips_hist_local puts in front (hist_local.c:301-306).
#ifndef VH_NBHD_TILE_H
#define VH_NBHD_TILE_H

#include "gcn.h"
#include "internal.h"

namespace vh {

// the order-preserving unsigned key of a float's bits, and back
VH_DEV unsigned int nb_float_key(unsigned int bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
VH_DEV unsigned int nb_float_unkey(unsigned int key) { return key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu); }

template <bool KEYF>
VH_DEV unsigned int nb_key(unsigned int dword, unsigned int key_xor)
{
	return KEYF ? nb_float_key(dword) ^ key_xor : dword ^ key_xor;
}
template <bool KEYF>
VH_DEV unsigned int nb_unkey(unsigned int key, unsigned int key_xor)
{
	return KEYF ? nb_float_unkey(key ^ key_xor) : key ^ key_xor;
}

template <int ES>
VH_DEV unsigned int nb_load_element(gptr_in row, unsigned int off)
{
	if constexpr (ES == 1)
		return gload8(row, off);
	else if constexpr (ES == 2)
		return gload16(row, off);
	else
		return gload32(row, off);
}

VH_DEV int nb_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
// vips_embed(VIPS_EXTEND_MIRROR) (conversion/embed.c): the image reflected about its edge, the edge pel repeated;
// one reflection (a window is never larger than the image), then the clamp for what nobody reads
VH_DEV int nb_mirror(int v, int size)
{
	v = v < 0 ? -1 - v : v >= size ? 2 * size - 1 - v : v;
	return nb_clamp(v, 0, size - 1);
}
template <bool MIRROR>
VH_DEV int nb_edge(int v, int size)
{
	return MIRROR ? nb_mirror(v, size) : nb_clamp(v, 0, size - 1);
}

// Stage `rows` rows, the first one image row y_start (before clamping), LDS byte 0 of each image element e_start.
// ES: bytes an element.  MIRROR: the edge is vips_embed's mirror instead of its copy (hist_local.hip).  Every thread
// of the block calls it; the caller puts the barrier behind it.
template <int ES, bool KEYF, bool MIRROR = false>
VH_DEV void nb_stage(const NbArgs &a, unsigned int *lds, int e_start, int y_start, int rows, int nthreads)
{
	constexpr int EPG = 16 / ES; // elements a 16-byte group
	const int groups = a.lds_row / 16;
	const int win_e0 = a.in_left * a.bands, win_e1 = (a.in_left + a.in_width) * a.bands;
	for (int idx = tid(); idx < rows * groups; idx += nthreads) {
		const int r = idx / groups, g = idx - r * groups;
		int y = nb_edge<MIRROR>(y_start + r, a.im_height);
		y = nb_clamp(y, a.in_top, a.in_top + a.in_height - 1);
		const unsigned long long row = (unsigned long long) a.in + (unsigned long long) (y - a.in_top) * (unsigned long long) a.in_stride;
		const gptr_in rowp = gptr_in_of(row);
		const int e0 = e_start + g * EPG;
		unsigned int w[4] = { 0, 0, 0, 0 };
		if (e0 >= win_e0 && e0 + EPG <= win_e1) {
			const unsigned int off = (unsigned int) (e0 - win_e0) * ES;
			if (((row + off) & 3) == 0)
				gload128(rowp, off, w);
			else {
#pragma unroll
				for (int k = 0; k < EPG; k++)
					w[(k * ES) >> 2] |= nb_load_element<ES>(rowp, off + k * ES) << (8 * ((k * ES) & 3));
			}
		}
		else {
#pragma unroll
			for (int k = 0; k < EPG; k++) {
				const int ee = e0 + k;
				int band = ee % a.bands;
				band = band < 0 ? band + a.bands : band;
				int pel = nb_edge<MIRROR>((ee - band) / a.bands, a.im_width);
				pel = nb_clamp(pel, a.in_left, a.in_left + a.in_width - 1);
				const unsigned int off = (unsigned int) ((pel - a.in_left) * a.bands + band) * ES;
				w[(k * ES) >> 2] |= nb_load_element<ES>(rowp, off) << (8 * ((k * ES) & 3));
			}
		}
		unsigned int *dst = lds + ((r * a.lds_row) >> 2) + 4 * g;
#pragma unroll
		for (int q = 0; q < 4; q++)
			dst[q] = nb_key<KEYF>(w[q], a.key_xor);
	}
}

} // namespace vh

#endif // VH_NBHD_TILE_H
