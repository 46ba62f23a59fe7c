// What the pointwise kernels of colour.hip and its parts (colour_cast.h, colour_sharpen.h, colour_premultiply.h) share: the rows a thread keeps in
// flight, the grid of a row-looping kernel, four elements as one aligned vector.
#pragma once

namespace vh {

// The pointwise kernels below give a thread one element column and RU rows per loop trip,
// all RU loads issued before the first is used: with one load in flight per thread these
// kernels sit at ~1 TB/s (bytes in flight, not bandwidth, bound them); four gets 3-4x.
constexpr int RU = 4;

// grid.y for a row-looping kernel: enough blocks to fill the part, few enough that per-block
// setup is amortised over many rows
static inline int rows_grid(int gx, int height)
{
	const int groups = (height + RU - 1) / RU;
	int gy = 16384 / (gx > 0 ? gx : 1);
	gy = gy < 1 ? 1 : gy;
	return groups < gy ? groups : gy;
}

// four elements that arrive as one aligned vector load and leave as one aligned vector store
template <typename T>
struct __attribute__((aligned(4 * sizeof(T)))) Vec4 {
	T v[4];
};

} // namespace vh
