// vips_mapim_gen (resample/mapim.c:307-428) for gfx950: a gather through an index image.  One thread makes one output
// pel: it reads its index pel, turns it into a coordinate of the embedded input or into the ink (the coordinate stage,
// mapim.c:228-305), and interpolates there with the nearest / bilinear / bicubic stencils of interp_device.h through
// EmbedFetch, the fetch of affine.hip: the vips_embed the build puts in front (mapim.c:472-479: the original at
// window_offset + 1, all six `extend` modes) is never materialised.
//
// Shape.  What a wave pays for is the cache lines it touches, in the index and in the input.  A wave is a 16 x 4 patch
// of the output, as in affine.hip: a row segment of a float index is one 128-byte line (a double index two, a short
// index half of one), and whatever the index does to neighbouring pels -- a rotation, a lens, a ripple -- the footprint
// of a compact patch in the input stays a compact patch of a few lines, where a 64 x 1 segment of a rotated image
// would cross a line every other pel.  An index pel is one load of its whole size (2 to 16 bytes) wherever its rows
// allow it.  The index format is a wave-uniform run-time switch in the load and in the coordinate stage: the kernels
// are image type x interpolator, 21 of them.
//
// Also here: vips_mapim_region_minmax (mapim.c:145-224) of a rect of the index as a read-only reduction, and vips_xyz
// (create/xyz.c) on the streaming grid of pointwise.h.
#include "interp_device.h"
#include "pointwise.h"

#include <climits>

namespace vh {

constexpr int MAPIM_BW = 16, MAPIM_BH = 16; // a block's patch of the output: waves of 16 x 4
constexpr int MAPIM_THREADS = POINTWISE_THREADS;
constexpr int MAPIM_BOUNDS_BLOCKS = POINTWISE_GRID_BLOCKS;

// Index pel i of a row: integer formats as px, py in d[0], d[1], sign- or zero-extended to 32 bits; float and complex
// their bits there; double and dpcomplex in d[0 .. 1], d[2 .. 3].  `wide`: one load of the whole pel.
VH_DEV void mapim_load_pel(gptr_in row, unsigned int i, int format, int wide, unsigned int (&d)[4])
{
	d[0] = d[1] = d[2] = d[3] = 0;
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR:
	case VIPS_HIP_FORMAT_CHAR: {
		const unsigned int v = wide ? gload16(row, 2u * i) : (unsigned int) gload8(row, 2u * i) | ((unsigned int) gload8(row, 2u * i + 1u) << 8);
		d[0] = v & 0xffu;
		d[1] = (v >> 8) & 0xffu;
		if (format == VIPS_HIP_FORMAT_CHAR) {
			d[0] = (unsigned int) (int) (signed char) d[0];
			d[1] = (unsigned int) (int) (signed char) d[1];
		}
		break;
	}
	case VIPS_HIP_FORMAT_USHORT:
	case VIPS_HIP_FORMAT_SHORT: {
		const unsigned int v = wide ? gload32(row, 4u * i) : gload16(row, 4u * i) | (gload16(row, 4u * i + 2u) << 16);
		d[0] = v & 0xffffu;
		d[1] = v >> 16;
		if (format == VIPS_HIP_FORMAT_SHORT) {
			d[0] = (unsigned int) (int) (short) d[0];
			d[1] = (unsigned int) (int) (short) d[1];
		}
		break;
	}
	case VIPS_HIP_FORMAT_UINT:
	case VIPS_HIP_FORMAT_INT:
	case VIPS_HIP_FORMAT_FLOAT:
	case VIPS_HIP_FORMAT_COMPLEX: {
		unsigned int w[2];
		gload64(row, 8u * i, w);
		d[0] = w[0];
		d[1] = w[1];
		break;
	}
	default:
		gload128(row, 16u * i, d);
		break;
	}
}

VH_DEV double mapim_double_of(unsigned int lo, unsigned int hi)
{
	return __builtin_bit_cast(double, (unsigned long long) lo | ((unsigned long long) hi << 32));
}

// The coordinate stage, mapim.c:228-305: true for the ink, else the embedded coordinate px + window_offset + 1 in the
// arithmetic of the index's type.  clip_width and clip_height are the EMBEDDED image's size less the stencil: the
// input's + 1.
VH_DEV bool mapim_coordinate(const MapimArgs &a, const unsigned int (&d)[4], double &x, double &y)
{
	const int cw = a.im_width + 1, ch = a.im_height + 1;
	const int wo = a.window_offset;
	switch (a.index_format) {
	case VIPS_HIP_FORMAT_UCHAR:
	case VIPS_HIP_FORMAT_USHORT:
	case VIPS_HIP_FORMAT_UINT:
		// ULOOKUP: the comparison and the sum are unsigned for uint (below clip_width they are the int's)
		if (d[0] >= (unsigned int) cw || d[1] >= (unsigned int) ch)
			return true;
		x = (double) ((int) d[0] + wo + 1);
		y = (double) ((int) d[1] + wo + 1);
		return false;
	case VIPS_HIP_FORMAT_CHAR:
	case VIPS_HIP_FORMAT_SHORT:
	case VIPS_HIP_FORMAT_INT: {
		// LOOKUP: -1 is let through for the antialiased edge
		const int px = (int) d[0], py = (int) d[1];
		if (px < -1 || px >= cw || py < -1 || py >= ch)
			return true;
		x = (double) (px + wo + 1);
		y = (double) (py + wo + 1);
		return false;
	}
	case VIPS_HIP_FORMAT_FLOAT:
	case VIPS_HIP_FORMAT_COMPLEX: {
		// FLOOKUP(float): the ints are converted to float, every sum is a float's
		const float px = __builtin_bit_cast(float, d[0]), py = __builtin_bit_cast(float, d[1]);
		if (px != px || py != py || px < -1.0f || px >= (float) cw || py < -1.0f || py >= (float) ch)
			return true;
		x = (double) __fadd_rn(__fadd_rn(px, (float) wo), 1.0f);
		y = (double) __fadd_rn(__fadd_rn(py, (float) wo), 1.0f);
		return false;
	}
	default: {
		const double px = mapim_double_of(d[0], d[1]), py = mapim_double_of(d[2], d[3]);
		if (px != px || py != py || px < -1.0 || px >= (double) cw || py < -1.0 || py >= (double) ch)
			return true;
		x = __dadd_rn(__dadd_rn(px, (double) wo), 1.0);
		y = __dadd_rn(__dadd_rn(py, (double) wo), 1.0);
		return false;
	}
	}
}

template <typename T, int INTERP>
__global__ void __launch_bounds__(MAPIM_BW * MAPIM_BH)
mapim_kernel(MapimArgs a)
{
	const int i = (int) blockIdx.x * MAPIM_BW + (int) threadIdx.x;
	const int yy = (int) blockIdx.y * MAPIM_BH + (int) threadIdx.y;
	if (i >= a.out_width || yy >= a.out_height)
		return;
	unsigned int d[4];
	mapim_load_pel(gptr_in_of((unsigned long long) a.index + (unsigned long long) yy * (unsigned long long) a.index_stride), (unsigned int) i,
		a.index_format, a.index_wide, d);
	double x = 0.0, y = 0.0;
	const bool ink = mapim_coordinate(a, d, x, y);
	T *q = (T *) (a.out + (long long) yy * a.out_stride) + (long long) i * a.bands;
	if (ink || a.in_width == 0) {
		for (int z = 0; z < a.bands; z++)
			q[z] = ((const T *) a.ink)[z];
		return;
	}
	interp_pel<T, INTERP>(q, x, y, a.bands, (const BicubicTables *) a.tables, EmbedFetch<T, MapimArgs>{a});
}

// ---------------------------------------------------------------------- the bounds pass

// One component of an index pel as a double: exact for every index format, so the extremes are those of the index's
// own type.
VH_DEV void mapim_components(int format, const unsigned int (&d)[4], double &px, double &py)
{
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR:
	case VIPS_HIP_FORMAT_USHORT:
	case VIPS_HIP_FORMAT_UINT:
		px = (double) d[0];
		py = (double) d[1];
		break;
	case VIPS_HIP_FORMAT_CHAR:
	case VIPS_HIP_FORMAT_SHORT:
	case VIPS_HIP_FORMAT_INT:
		px = (double) (int) d[0];
		py = (double) (int) d[1];
		break;
	case VIPS_HIP_FORMAT_FLOAT:
	case VIPS_HIP_FORMAT_COMPLEX:
		px = (double) __builtin_bit_cast(float, d[0]);
		py = (double) __builtin_bit_cast(float, d[1]);
		break;
	default:
		px = mapim_double_of(d[0], d[1]);
		py = mapim_double_of(d[2], d[3]);
		break;
	}
}

// mapim.c:207-218: VIPS_CLIP(-1, v, VIPS_MAX_COORD) of the rounded extreme, as an int
VH_DEV int mapim_clip_coord(double v)
{
	v = v > (double) MAPIM_MAX_COORD ? (double) MAPIM_MAX_COORD : v;
	v = v < -1.0 ? -1.0 : v;
	return vh::cvt_i32(v);
}

// Blocks take rows in turns, a block's lanes a row's pels in turns; the block's extremes meet in LDS and leave as
// four integer atomics (min x, min y, max x, max y: floor, ceil and the clip are monotonic, so they commute with the
// extremes).  A component that is NaN is skipped, and a component with no number at all sends nothing.
__global__ void __launch_bounds__(MAPIM_THREADS)
mapim_bounds_kernel(const unsigned char *index, long long index_stride, int width, int height, int format, int wide, int *bounds)
{
	__shared__ double s_lo[2][MAPIM_THREADS];
	__shared__ double s_hi[2][MAPIM_THREADS];
	const double inf = __builtin_huge_val();
	double lo_x = inf, lo_y = inf, hi_x = -inf, hi_y = -inf;
	const int t = (int) threadIdx.x;
	for (int yy = (int) blockIdx.y; yy < height; yy += (int) gridDim.y) {
		const gptr_in row = gptr_in_of((unsigned long long) index + (unsigned long long) yy * (unsigned long long) index_stride);
		for (int i = (int) blockIdx.x * MAPIM_THREADS + t; i < width; i += (int) gridDim.x * MAPIM_THREADS) {
			unsigned int d[4];
			mapim_load_pel(row, (unsigned int) i, format, wide, d);
			double px, py;
			mapim_components(format, d, px, py);
			// (a comparison with a NaN is false: it changes nothing)
			lo_x = px < lo_x ? px : lo_x;
			hi_x = px > hi_x ? px : hi_x;
			lo_y = py < lo_y ? py : lo_y;
			hi_y = py > hi_y ? py : hi_y;
		}
	}
	s_lo[0][t] = lo_x;
	s_lo[1][t] = lo_y;
	s_hi[0][t] = hi_x;
	s_hi[1][t] = hi_y;
	__syncthreads();
	for (int step = MAPIM_THREADS / 2; step > 0; step >>= 1) {
		if (t < step) {
			for (int c = 0; c < 2; c++) {
				s_lo[c][t] = s_lo[c][t + step] < s_lo[c][t] ? s_lo[c][t + step] : s_lo[c][t];
				s_hi[c][t] = s_hi[c][t + step] > s_hi[c][t] ? s_hi[c][t + step] : s_hi[c][t];
			}
		}
		__syncthreads();
	}
	if (t < 2 && s_lo[t][0] <= s_hi[t][0]) {
		atomicMin(bounds + t, mapim_clip_coord(floor(s_lo[t][0])));
		atomicMax(bounds + 2 + t, mapim_clip_coord(ceil(s_hi[t][0])));
	}
}

// ---------------------------------------------------------------------- xyz

// create/xyz.c:77-103 in two dimensions: a lane makes the 16-byte groups -- two pels -- of the rows in turns
__global__ void __launch_bounds__(MAPIM_THREADS)
xyz_kernel(unsigned char *out, long long out_stride, int width, int height, int groups)
{
	const unsigned int total = (unsigned int) groups * (unsigned int) height;
	for (unsigned int at = (unsigned int) blockIdx.x * MAPIM_THREADS + (unsigned int) threadIdx.x; at < total; at += (unsigned int) gridDim.x * MAPIM_THREADS) {
		const unsigned int y = at / (unsigned int) groups;
		const unsigned int g = at - y * (unsigned int) groups;
		const unsigned int x = 2u * g;
		const gptr_out p = gptr_out_of((unsigned long long) out + (unsigned long long) y * (unsigned long long) out_stride) + g * (unsigned int) POINTWISE_GROUP;
		if (x + 1u < (unsigned int) width) {
			const unsigned int w[4] = { x, y, x + 1u, y };
			gstore128(p, w);
		}
		else {
			// the last pel of an odd row
			const unsigned int w[2] = { x, y };
			gstore_dwords<2>(p, w);
		}
	}
}

// ---------------------------------------------------------------------- host side

template <typename T>
static int mapim_launch(const MapimArgs &a, int interpolate)
{
	const dim3 block(MAPIM_BW, MAPIM_BH, 1);
	const dim3 grid((a.out_width + MAPIM_BW - 1) / MAPIM_BW, (a.out_height + MAPIM_BH - 1) / MAPIM_BH, 1);
	if (interpolate == VIPS_HIP_INTERPOLATE_NEAREST) {
		Gate gate("mapim_nearest");
		hipLaunchKernelGGL((mapim_kernel<T, 0>), grid, block, 0, stream(), a);
	}
	else if (interpolate == VIPS_HIP_INTERPOLATE_BILINEAR) {
		Gate gate("mapim_bilinear");
		hipLaunchKernelGGL((mapim_kernel<T, 1>), grid, block, 0, stream(), a);
	}
	else {
		Gate gate("mapim_bicubic");
		hipLaunchKernelGGL((mapim_kernel<T, 2>), grid, block, 0, stream(), a);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

// the rows of an index let a lane read its pel in one load: 2- and 4-byte pels on multiples of their size, wider ones
// on dwords (which whole elements give them)
static int mapim_index_wide(const void *index, long long stride, int format)
{
	const int pel = 2 * format_sizeof(format_real(format));
	return on_unit(index, stride, (uintptr_t) (pel < 4 ? pel : 4)) ? 1 : 0;
}

// Everything about the regions has been checked (ops_mapim.cpp).
int mapim_run(const char *domain, MapimArgs a, int format, int interpolate)
{
	if (a.out_width < 1 || a.out_height < 1)
		return 0;
	if ((a.out_height + MAPIM_BH - 1) / MAPIM_BH > 65535 || a.out_width > (1 << 27)) {
		error(domain, "image too large");
		return -1;
	}
	a.index_wide = mapim_index_wide(a.index, a.index_stride, a.index_format);
	a.tables = bicubic_tables();
	if (!a.tables)
		return -1;
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR: return mapim_launch<unsigned char>(a, interpolate);
	case VIPS_HIP_FORMAT_CHAR: return mapim_launch<signed char>(a, interpolate);
	case VIPS_HIP_FORMAT_USHORT: return mapim_launch<unsigned short>(a, interpolate);
	case VIPS_HIP_FORMAT_SHORT: return mapim_launch<short>(a, interpolate);
	case VIPS_HIP_FORMAT_UINT: return mapim_launch<unsigned int>(a, interpolate);
	case VIPS_HIP_FORMAT_INT: return mapim_launch<int>(a, interpolate);
	case VIPS_HIP_FORMAT_FLOAT: return mapim_launch<float>(a, interpolate);
	default: break;
	}
	error(domain, "band format %d is outside the HIP path", format);
	return -1;
}

int mapim_bounds_run(const char *domain, const unsigned char *index, long long index_stride, int width, int height, int index_format,
	int *bounds)
{
	if (width < 1 || height < 1 || width > (1 << 27)) {
		error(domain, "bad index rect");
		return -1;
	}
	// the minima start above and the maxima below every clipped coordinate
	VH_CHECK(hipMemsetAsync(bounds, 0x7f, 2 * sizeof(int), stream()));
	VH_CHECK(hipMemsetAsync(bounds + 2, 0x80, 2 * sizeof(int), stream()));
	const int bx = (width + MAPIM_THREADS - 1) / MAPIM_THREADS;
	const dim3 grid(bx < MAPIM_BOUNDS_BLOCKS ? bx : MAPIM_BOUNDS_BLOCKS, pointwise_rows_grid(bx, height), 1);
	{
		Gate gate("mapim_bounds");
		hipLaunchKernelGGL(mapim_bounds_kernel, grid, dim3(MAPIM_THREADS, 1, 1), 0, stream(), index, index_stride, width, height,
			index_format, mapim_index_wide(index, index_stride, index_format), bounds);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

int xyz_run(const char *domain, unsigned char *out, long long out_stride, int width, int height)
{
	const long long groups = ((long long) width + 1) / 2;
	if (width < 1 || height < 1 || groups * height >= (1LL << 31)) {
		error(domain, "image too large");
		return -1;
	}
	{
		Gate gate("xyz");
		hipLaunchKernelGGL(xyz_kernel, pointwise_stream_grid(groups * height), dim3(MAPIM_THREADS, 1, 1), 0, stream(), out, out_stride, width,
			height, (int) groups);
	}
	VH_CHECK(hipGetLastError());
	return 0;
}

int mapim_tile(int what)
{
	switch (what) {
	case 0: return MAPIM_BW;
	case 1: return MAPIM_BH;
	case 2: return 16;
	case 3: return 64 / 16;
	case 4: return MAPIM_BOUNDS_BLOCKS;
	case 5: return MAPIM_THREADS;
	case 6: return POINTWISE_GROUP;
	case 7: return POINTWISE_GRID_BLOCKS;
	default: return -1;
	}
}

} // namespace vh
