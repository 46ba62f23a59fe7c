// Host side of the uchar reduce kernels on the matrix cores: is a plan's geometry regular, its taps as the kernels
// want them, the A-operand tables and where they are kept.
#pragma once

#include "reduce_u8.h"
#include "reduce_u8_device.h"

#include <cstring>
#include <mutex>
#include <tuple>
#include <vector>

namespace vh {

// Is pos[] an arithmetic progression first0 + S*k with one phase?  (What an
// integer shrink of a size-divisible image produces.)
static bool positions_regular(const std::vector<ReducePos> &pos, int *first0, int *step, int *phase)
{
	if (pos.empty())
		return false;
	*first0 = pos[0].first;
	*phase = pos[0].phase;
	*step = pos.size() > 1 ? pos[1].first - pos[0].first : 0;
	for (size_t k = 0; k < pos.size(); k++)
		if (pos[k].first != *first0 + (int) k * *step || pos[k].phase != *phase)
			return false;
	return true;
}

// Pack taps [0, n) of matrixs row `phase`, zero-padded to `total`, as i16 pairs.
static void pack_pairs(const _VipsHipReduce *r, int phase, int total, std::vector<unsigned int> &out)
{
	const short *c = &r->matrixs[(size_t) phase * r->n_point];
	out.resize(total / 2);
	for (int q = 0; q < total / 2; q++) {
		const int k0 = 2 * q, k1 = 2 * q + 1;
		const unsigned short lo = k0 < r->n_point ? (unsigned short) c[k0] : 0;
		const unsigned short hi = k1 < r->n_point ? (unsigned short) c[k1] : 0;
		out[q] = (unsigned int) lo | ((unsigned int) hi << 16);
	}
}

// number of leading taps that matter: trailing zero coefficients are dropped
static int effective_taps(const _VipsHipReduce *r, int phase)
{
	const short *c = &r->matrixs[(size_t) phase * r->n_point];
	int n = r->n_point;
	while (n > 1 && c[n - 1] == 0)
		n--;
	return n;
}

// f16 bit pattern of an integer |v| < 2048 (exact)
static unsigned short half_bits(int v)
{
	const _Float16 h = (_Float16) (float) v;
	unsigned short bits;
	memcpy(&bits, &h, sizeof(bits));
	return bits;
}

// The MFMA kernel's A-operand tables (both walking directions) for taps c[0 .. 8*D).
static void mfma_build_tables(const std::vector<int> &taps, const std::vector<int> &taps_h, int D,
	MfmaTables *tab)
{
	const int nt = 8 * D;
	for (int rot = 0; rot < MFMA_SLOTS; rot++)
		for (int q = 0; q < 2; q++)
			for (int h = 0; h < 2; h++)
				for (int i = 0; i < 4; i++) {
					const int d = (rot - (4 * h + i) + 2 * MFMA_SLOTS) % MFMA_SLOTS;
					for (int k = 0; k < 4; k++)
						tab->ah[((((rot * 2 + q) * 2 + h) * 4 + i) * 4) + k] =
							half_bits(d < D ? taps_h[8 * d + 4 * q + k] : 0);
				}
	for (int flip = 0; flip < 2; flip++)
		for (int rot = 0; rot < MFMA_SLOTS; rot++)
			for (int q = 0; q < 2; q++)
				for (int h = 0; h < 2; h++)
					for (int i = 0; i < 4; i++) {
						const int slot = 4 * h + i;
						const int d = (rot - slot + 2 * MFMA_SLOTS) % MFMA_SLOTS;
						for (int k = 0; k < 4; k++) {
							int c = 0;
							if (d < D) {
								const int tap = 8 * d + 4 * q + k;
								c = flip ? taps[nt - 1 - tap] : taps[tap];
							}
							tab->a[flip][((((rot * 2 + q) * 2 + h) * 4 + i) * 4) + k] = half_bits(c);
						}
					}
}

// Taps [0, 8 * D) of coefficient row `phase`, zero-padded.  False when the matrix kernels would not be exact with them:
// |c| < 2048 is an exact half, sum |c| * 255 < 2^23 keeps 2n + 1 in 24 bits (reduce_u8_device.h).
static bool mfma_taps(const _VipsHipReduce *r, int phase, int D, std::vector<int> &taps)
{
	const short *c = &r->matrixs[(size_t) phase * r->n_point];
	taps.assign(8 * D, 0);
	long long abs_sum = 0;
	int abs_max = 0;
	for (int k = 0; k < 8 * D; k++) {
		if (k < r->n_point)
			taps[k] = c[k];
		const int av = taps[k] < 0 ? -taps[k] : taps[k];
		abs_sum += av;
		abs_max = av > abs_max ? av : abs_max;
	}
	return abs_max < 2048 && abs_sum * 255 < (1 << 23);
}

// The device copy of the tables for these taps, kept with the plan's other device tables (pos_cache, freed with the
// plan) under `key`; built and uploaded on first use.  nullptr: the upload failed.
static const MfmaTables *mfma_tables_cached(_VipsHipReduce *r, std::tuple<int, int, int> key, const std::vector<int> &taps_v,
	const std::vector<int> &taps_h, int D)
{
	std::lock_guard<std::mutex> lock(r->mutex);
	auto it = r->pos_cache.find(key);
	if (it != r->pos_cache.end())
		return (const MfmaTables *) it->second;
	MfmaTables tab;
	mfma_build_tables(taps_v, taps_h, D, &tab);
	void *d = upload(&tab, sizeof(tab));
	if (d)
		r->pos_cache[key] = (ReducePos *) d;
	return (const MfmaTables *) d;
}

// reduce_fused_exch.hip: the fused RGBA reduce on tiles without a horizontal halo; 0 launched, 1 not this kernel's
// case, -1 error
struct FusedArgs;
int launch_fused_mfma_x(const FusedArgs &all, const VipsHipRegion *in, const VipsHipRegion *out, const MfmaTables *d_tables);
// reduce_fused_u8x3.hip: the fused reduce of three interleaved bands; 0 launched, 1 not this kernel's case, -1 error
int launch_fused_u8x3(int D, int taps_h, const VipsHipRegion *in, const VipsHipRegion *out, int fx0, int fy0,
	const MfmaTables *d_tables);

} // namespace vh
