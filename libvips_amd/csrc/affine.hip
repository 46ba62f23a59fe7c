// vips_affine_gen (resample/affine.c:226-410) for gfx950: any matrix, the nearest / bilinear / bicubic interpolators
// (interp_device.h, shared with upsize.hip), the clip against the input area with the background ink, and the six
// `extend` modes of the vips_embed the build puts in front (conversion/embed.c) -- never materialised: an embedded
// coordinate becomes a source pel or the fill pel in the fetch.
//
// Coordinates.  The reference computes the input coordinate of a generate rect's first pixel of every row from
// scratch and then ACCUMULATES `ix += ddx; iy += ddy` along the row, so a pixel's coordinates depend on where its rect
// starts: with vips_image_write_to_memory the rects of a SMALLTILE image are the sink's 128 x 128 tiles on the output
// image's grid.  start + k * ddx is another number (at 45 degrees a few hundred floor()s per million pixels differ), so
// the accumulation is replayed: a thread owns one output pixel, computes its row's start as the reference does and
// repeats its column-in-tile adds, up to 127 pairs of dependent v_add_f64.  A wave is a 16 x 4 patch of the output:
// its lanes' replay lengths differ by at most 15 and a rotated footprint stays within a few cache lines.
// With whole-row rects (b == c == 0: ddy is a zero, y does not move) the x of a column comes from a table the host
// replays once, as in upsize.hip.
#include "interp_device.h"

#include <cstring>
#include <list>
#include <memory>
#include <mutex>
#include <vector>

namespace vh {

constexpr int AFFINE_BW = 16, AFFINE_BH = 16; // a block's patch of the output: waves of 16 x 4

// (the fetch through the six extend modes: EmbedFetch, interp_device.h, shared with mapim.hip)
template <typename T>
using AffineFetch = EmbedFetch<T, AffineArgs>;

template <typename T, int INTERP>
__global__ void __launch_bounds__(AFFINE_BW * AFFINE_BH)
affine_kernel(AffineArgs a)
{
	const int i = blockIdx.x * AFFINE_BW + threadIdx.x;
	const int yy = blockIdx.y * AFFINE_BH + threadIdx.y;
	if (i >= a.out_width || yy >= a.out_height)
		return;
	const int wo = a.window_offset;
	const int col = a.out_left + i;
	// affine.c:340-362, the rect this pixel is in starting at column le
	const int le = a.tile_width > 0 ? col / a.tile_width * a.tile_width : 0;
	const double ox = __dsub_rn((double) (le + a.oarea_left), a.odx);
	const double oy = __dsub_rn((double) (a.out_top + yy + a.oarea_top), a.ody);
	double x = __dadd_rn(__dmul_rn(a.ia, ox), __dmul_rn(a.ib, oy));
	double y = __dadd_rn(__dmul_rn(a.ic, ox), __dmul_rn(a.id, oy));
	x = __dsub_rn(x, a.tidx);
	y = __dsub_rn(y, a.tidy);
	x = __dadd_rn(x, (double) wo);
	y = __dadd_rn(y, (double) wo);
	if (a.tile_width > 0) {
		// affine.c:399-400, once per pixel to the left in this rect
		for (int k = col - le; k > 0; k--) {
			x = __dadd_rn(x, a.ia);
			y = __dadd_rn(y, a.ic);
		}
	}
	else
		x = a.tabx[i]; // (ddy is a zero: y stays)

	// affine.c:328-331, :369-377: the clip rectangle in embedded coordinates, both ends inclusive
	const int ile = wo, ito = wo, iri = wo + a.im_width, ibo = wo + a.im_height;
	const int fx = vh::cvt_i32(floor(x));
	const int fy = vh::cvt_i32(floor(y));
	T *q = (T *) (a.out + (long long) yy * a.out_stride) + (long long) i * a.bands;
	if (a.in_width == 0 || !(fx >= ile && fx <= iri && fy >= ito && fy <= ibo)) {
		for (int z = 0; z < a.bands; z++)
			q[z] = ((const T *) a.ink)[z];
		return;
	}
	interp_pel<T, INTERP>(q, x, y, a.bands, (const BicubicTables *) a.tables, AffineFetch<T>{a});
}

// ---------------------------------------------------------------------- host side

// the per-column x coordinates of whole-row rects, cached (a table upload synchronises the stream)
struct AffineTabKey {
	int device, out_left, out_width, window_offset, oarea_left;
	double ia, odx, tidx;
	bool operator==(const AffineTabKey &o) const
	{
		return device == o.device && out_left == o.out_left && out_width == o.out_width && window_offset == o.window_offset &&
			oarea_left == o.oarea_left && memcmp(&ia, &o.ia, sizeof(double)) == 0 && memcmp(&odx, &o.odx, sizeof(double)) == 0 &&
			memcmp(&tidx, &o.tidx, sizeof(double)) == 0;
	}
};
typedef std::shared_ptr<double> AffineTabPtr;
static std::mutex &g_affine_mutex = *new std::mutex;
static std::list<std::pair<AffineTabKey, AffineTabPtr>> &g_affine_tabs = *new std::list<std::pair<AffineTabKey, AffineTabPtr>>;

static AffineTabPtr affine_column_table(const AffineTabKey &key)
{
	{
		std::lock_guard<std::mutex> lock(g_affine_mutex);
		for (auto it = g_affine_tabs.begin(); it != g_affine_tabs.end(); ++it)
			if (it->first == key) {
				g_affine_tabs.splice(g_affine_tabs.begin(), g_affine_tabs, it);
				return g_affine_tabs.front().second;
			}
	}
	// affine.c:340-400 for a rect that starts at column 0 (ib * oy is a zero)
	std::vector<double> tab(key.out_width);
	double x = key.ia * ((double) key.oarea_left - key.odx);
	x -= key.tidx;
	x += key.window_offset;
	for (int xx = 0; xx < key.out_left + key.out_width; xx++) {
		if (xx >= key.out_left)
			tab[xx - key.out_left] = x;
		x += key.ia;
	}
	double *d = (double *) upload(tab.data(), tab.size() * sizeof(double));
	if (!d)
		return AffineTabPtr();
	AffineTabPtr p(d, [](double *q) { vips_hip_free(q); });
	std::lock_guard<std::mutex> lock(g_affine_mutex);
	g_affine_tabs.emplace_front(key, p);
	while (g_affine_tabs.size() > 32)
		g_affine_tabs.pop_back();
	return p;
}

template <typename T>
static int affine_launch(const AffineArgs &a, int interpolate)
{
	const dim3 block(AFFINE_BW, AFFINE_BH, 1);
	const dim3 grid((a.out_width + AFFINE_BW - 1) / AFFINE_BW, (a.out_height + AFFINE_BH - 1) / AFFINE_BH, 1);
	if (interpolate == VIPS_HIP_INTERPOLATE_NEAREST) {
		Gate gate("affine_nearest");
		hipLaunchKernelGGL((affine_kernel<T, 0>), grid, block, 0, stream(), a);
	}
	else if (interpolate == VIPS_HIP_INTERPOLATE_BILINEAR) {
		Gate gate("affine_bilinear");
		hipLaunchKernelGGL((affine_kernel<T, 1>), grid, block, 0, stream(), a);
	}
	else {
		Gate gate("affine_bicubic");
		hipLaunchKernelGGL((affine_kernel<T, 2>), grid, block, 0, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

// Everything about the regions has been checked (ops_affine.cpp).
int affine_run(const char *domain, AffineArgs a, int format, int interpolate)
{
	if (a.out_width < 1 || a.out_height < 1)
		return 0;
	if ((a.out_height + AFFINE_BH - 1) / AFFINE_BH > 65535) {
		error(domain, "image too large");
		return -1;
	}
	AffineTabPtr tab;
	a.tabx = nullptr;
	if (a.tile_width == 0) {
		AffineTabKey key;
		memset(&key, 0, sizeof(key));
		key.device = current_device();
		key.out_left = a.out_left;
		key.out_width = a.out_width;
		key.window_offset = a.window_offset;
		key.oarea_left = a.oarea_left;
		key.ia = a.ia;
		key.odx = a.odx;
		key.tidx = a.tidx;
		tab = affine_column_table(key);
		if (!tab)
			return -1;
		a.tabx = tab.get();
	}
	a.tables = bicubic_tables();
	if (!a.tables)
		return -1;
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR: return affine_launch<unsigned char>(a, interpolate);
	case VIPS_HIP_FORMAT_CHAR: return affine_launch<signed char>(a, interpolate);
	case VIPS_HIP_FORMAT_USHORT: return affine_launch<unsigned short>(a, interpolate);
	case VIPS_HIP_FORMAT_SHORT: return affine_launch<short>(a, interpolate);
	case VIPS_HIP_FORMAT_UINT: return affine_launch<unsigned int>(a, interpolate);
	case VIPS_HIP_FORMAT_INT: return affine_launch<int>(a, interpolate);
	case VIPS_HIP_FORMAT_FLOAT: return affine_launch<float>(a, interpolate);
	default: break;
	}
	error(domain, "band format %d is outside the HIP path", format);
	return -1;
}

} // namespace vh
