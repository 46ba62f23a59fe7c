// vips_morph (morphology/morph.c): erode and dilate of uchar images by a mask of 0, 128 and 255, on the device
// (gfx950).  The reference's C loops (morph.c:717-731, 804-818) run over ELEMENTS and are bitwise: dilate ORs, erode
// ANDs, over every mask position that is not 128, the input byte (255) or its complement (0).  Nothing compares:
// an input byte of 0x0f comes through as bits.
//
//   morph_erode / morph_dilate   A block of 256 threads makes MORPH_TW = 1024 elements x MORPH_TH = 16 rows from a
//                  halo tile in LDS (nbhd_tile.h).  A lane owns one DWORD of a row -- four elements -- so a mask
//                  position is a byte-shifted read of an LDS row: two aligned dwords and a funnel shift by a
//                  wave-uniform amount, then AND / OR / NOT on all four bytes at once.  The 128s are dropped on the
//                  host: the mask arrives as two bit rows a mask row (which columns keep the byte, which invert
//                  it), in the kernel arguments, and the kernel walks the set bits with scalar instructions.  The
//                  bit rows are read where they lie, a scalar load a mask row (a by-value array indexed at run time
//                  would be copied to scratch; all 64 dwords held in registers leave the rest too few of them).
//
// Masks are at most MORPH_MAX_SIDE = 32 on a side (a bit row is a dword) and the tile must fit a CU's 160 KB of LDS,
// which it does up to 76 bands at 32 x 32; the host refuses the rest.
#include "nbhd_tile.h"

#include <cstddef>
#include <cstdint>

namespace vh {

constexpr int MORPH_THREADS = 256;
constexpr int MORPH_TW = 4 * MORPH_THREADS; // elements = bytes
constexpr int MORPH_TH = 16;                // rows
constexpr int MORPH_MAX_SIDE = 32;
constexpr int MORPH_LDS_MAX = 160 * 1024; // a CU's LDS

struct MorphArgs {
	NbArgs nb;
	unsigned int rows[2 * MORPH_MAX_SIDE]; // bit i of [2 j]: mask (i, j) is 255; of [2 j + 1]: it is 0
};

// dword `index` of the bit rows, from the kernel argument segment
VH_DEV unsigned int morph_mask_word(int index)
{
	typedef const unsigned int __attribute__((address_space(4))) *Words;
	const Words w = (Words) ((const char __attribute__((address_space(4))) *) __builtin_amdgcn_kernarg_segment_ptr() +
		offsetof(MorphArgs, rows));
	return w[index];
}

template <bool DILATE>
__global__ void __launch_bounds__(MORPH_THREADS)
morph_kernel(MorphArgs m)
{
	VH_DYNAMIC_LDS(unsigned int, lds);
	const NbArgs &a = m.nb;

	const int out_e0 = a.out_left * a.bands + (int) blockIdx.x * MORPH_TW;
	const int y0 = (int) blockIdx.y * MORPH_TH;
	const int s = out_e0 - (a.win_w / 2) * a.bands;
	const int s_al = s & ~3;
	const int lead = s - s_al;
	nb_stage<1, false>(a, lds, s_al, a.out_top + y0 - a.win_h / 2, MORPH_TH + a.win_h - 1, MORPH_THREADS);
	barrier();

	const int t = tid();
	const int e = (int) blockIdx.x * MORPH_TW + 4 * t; // the lane's first element, of the output rect's row
	const int out_elems = a.out_width * a.bands;
	const int row_dwords = a.lds_row >> 2;
	for (int ty = 0; ty < MORPH_TH; ty++) {
		if (y0 + ty >= a.out_height)
			break;
		unsigned int acc = DILATE ? 0u : 0xffffffffu;
		for (int j = 0; j < a.win_h; j++) {
			const unsigned int invert = morph_mask_word(2 * j + 1);
			unsigned int bits = morph_mask_word(2 * j) | invert;
			const unsigned int *row = lds + (ty + j) * row_dwords + t;
			while (bits) {
				const int i = __builtin_ctz(bits);
				bits &= bits - 1;
				const int o = lead + i * a.bands;
				const unsigned long long both = ((unsigned long long) row[(o >> 2) + 1] << 32) | row[o >> 2];
				unsigned int v = (unsigned int) (both >> (8 * (o & 3)));
				v = (invert >> i) & 1 ? ~v : v;
				acc = DILATE ? acc | v : acc & v;
			}
		}
		if (e < out_elems) {
			const unsigned long long p = (unsigned long long) a.out + (unsigned long long) (y0 + ty) * (unsigned long long) a.out_stride +
				(unsigned long long) e;
			if ((p & 3) == 0 && e + 4 <= out_elems)
				gstore32(gptr_out_of(p), acc);
			else {
#pragma unroll
				for (int k = 0; k < 4; k++)
					if (e + k < out_elems)
						gstore8(gptr_out_of(p + k), (unsigned char) (acc >> (8 * k)));
			}
		}
	}
}

// Everything about the regions has been checked (ops_morphology.cpp); `mask` holds 0, 128 and 255 only.
int morph_run(const char *domain, NbArgs a, const unsigned char *mask, int dilate)
{
	if (a.win_w > MORPH_MAX_SIDE || a.win_h > MORPH_MAX_SIDE) {
		error(domain, "a %d x %d mask: the kernel takes masks up to %d x %d", a.win_w, a.win_h, MORPH_MAX_SIDE, MORPH_MAX_SIDE);
		return -1;
	}
	// the lead of the rounding, the tile, the halo, the dword behind the last one read
	const long long row = (3 + MORPH_TW + (long long) (a.win_w - 1) * a.bands + 4 + 15) / 16 * 16;
	const long long lds = row * (MORPH_TH + a.win_h - 1);
	if (lds > MORPH_LDS_MAX) {
		error(domain, "a %d x %d mask on %d-band images needs %lld KB of LDS, the kernel has %d", a.win_w, a.win_h, a.bands,
			(lds + 1023) / 1024, MORPH_LDS_MAX / 1024);
		return -1;
	}
	MorphArgs m = {};
	a.lds_row = (int) row;
	a.key_xor = 0;
	a.index = 0;
	m.nb = a;
	for (int j = 0; j < a.win_h; j++)
		for (int i = 0; i < a.win_w; i++) {
			const unsigned char c = mask[j * a.win_w + i];
			if (c == 255)
				m.rows[2 * j] |= 1u << i;
			else if (c == 0)
				m.rows[2 * j + 1] |= 1u << i;
		}
	const long long out_elems = (long long) a.out_width * a.bands;
	const dim3 grid((unsigned int) ((out_elems + MORPH_TW - 1) / MORPH_TW), (unsigned int) ((a.out_height + MORPH_TH - 1) / MORPH_TH), 1);
	const auto kernel = dilate ? morph_kernel<true> : morph_kernel<false>;
	if (lds > 64 * 1024)
		VH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MORPH_LDS_MAX));
	{
		Gate gate(dilate ? "morph_dilate" : "morph_erode");
		hipLaunchKernelGGL(kernel, grid, dim3(MORPH_THREADS), (size_t) lds, stream(), m);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

int morph_tile(int what)
{
	return what == 0 ? MORPH_TW : what == 1 ? MORPH_TH : what == 2 ? MORPH_MAX_SIDE : 0;
}

} // namespace vh
