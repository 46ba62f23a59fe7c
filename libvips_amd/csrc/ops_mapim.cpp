// vips_mapim (resample/mapim.c) and vips_xyz (create/xyz.c) on images in HBM: the host side -- the checks of
// vips_mapim_build, the ink and the fill pel (shared with vips_affine, ops_affine.cpp), the need of a generate rect
// (mapim.c:145-224, :351-365) from the bounds the device finds, the region checks, the premultiply chain, the C ABI.
// The kernels are in mapim.hip.
#include "internal.h"

#include <cmath>
#include <cstring>

using namespace vh;

namespace {

const char *MAPIM_DOMAIN = "mapim";

// vips_check_twocomponents (iofuncs/error.c:713-723); and what the reference takes and walks wrongly (p1 += 2)
int check_index(int bands, int format)
{
	if (format_sizeof(format) == 0) {
		error(MAPIM_DOMAIN, "unknown band format %d of the index", format);
		return -1;
	}
	if (!format_iscomplex(format) && bands != 2) {
		error(MAPIM_DOMAIN, "image must be two-band or complex");
		return -1;
	}
	if (format_iscomplex(format) && bands != 1) {
		error(MAPIM_DOMAIN, "a complex index of more than one band is outside the HIP path");
		return -1;
	}
	return 0;
}

int check_args(const VipsHipMapim *args, int format)
{
	return resample_check(MAPIM_DOMAIN, args->interpolate, args->extend, format);
}

bool on_elements(const VipsHipRegion *r)
{
	const size_t es = (size_t) format_sizeof(format_real(r->format));
	return ((size_t) (uintptr_t) r->data | r->stride) % es == 0;
}

// VIPS_CLIP(-1, v, VIPS_MAX_COORD)
double clip_coord(double v)
{
	const double m = (double) MAPIM_MAX_COORD < v ? (double) MAPIM_MAX_COORD : v;
	return -1.0 > m ? -1.0 : m;
}

// The regions are checked, the pels made: the need of the rect against the window, then the launch.
int gen_checked(const VipsHipRegion *in, const VipsHipRegion *index, const VipsHipRegion *out, const VipsHipMapim *args,
	const ResamplePels &pels, int in_width, int in_height)
{
	const bool whole = in->left == 0 && in->top == 0 && in->width == in_width && in->height == in_height;
	bool all_ink = false;
	if (!whole) {
		int need[4];
		if (vips_hip_mapim_need(index, args, in_width, in_height, need))
			return -1;
		all_ink = need[2] == 0 || need[3] == 0;
		if (!all_ink && (need[0] < in->left || need[1] < in->top || need[0] + need[2] > in->left + in->width ||
							need[1] + need[3] > in->top + in->height)) {
			error(MAPIM_DOMAIN, "input region too small");
			return -1;
		}
	}
	MapimArgs a;
	memset(&a, 0, sizeof(a));
	a.in = (const unsigned char *) in->data;
	a.index = (const unsigned char *) index->data;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.index_stride = (long long) index->stride;
	a.out_stride = (long long) out->stride;
	a.in_left = in->left;
	a.in_top = in->top;
	a.in_width = all_ink ? 0 : in->width;
	a.in_height = all_ink ? 0 : in->height;
	a.im_width = in_width;
	a.im_height = in_height;
	a.out_width = out->width;
	a.out_height = out->height;
	a.bands = in->bands;
	a.index_format = index->format;
	a.window_offset = pels.window_offset;
	a.extend = args->extend;
	memcpy(a.ink, pels.ink, sizeof(a.ink));
	memcpy(a.fill, pels.fill, sizeof(a.fill));
	return mapim_run(MAPIM_DOMAIN, a, in->format, args->interpolate);
}

// what vips_hip_mapim_gen checks of its regions, for the whole-image form too
int check_regions(const VipsHipRegion *in, const VipsHipRegion *index, const VipsHipRegion *out, int in_width, int in_height)
{
	if (check_region(MAPIM_DOMAIN, in) || check_region(MAPIM_DOMAIN, index) || check_region(MAPIM_DOMAIN, out))
		return -1;
	if (in_width < 1 || in_height < 1 || in->im_width != in_width || in->im_height != in_height) {
		error(MAPIM_DOMAIN, "the input region must belong to the in_width x in_height image");
		return -1;
	}
	if (out->format != in->format || out->bands != in->bands) {
		error(MAPIM_DOMAIN, "the output region must have the input's bands and format");
		return -1;
	}
	if (out->left != index->left || out->top != index->top || out->width != index->width || out->height != index->height ||
		out->im_width != index->im_width || out->im_height != index->im_height) {
		error(MAPIM_DOMAIN, "the output region must be the index region's rect");
		return -1;
	}
	const VipsHipRegion *all[3] = { in, index, out };
	for (const VipsHipRegion *r : all) {
		if (r->left < 0 || r->top < 0 || (long long) r->left + r->width > r->im_width || (long long) r->top + r->height > r->im_height) {
			error(MAPIM_DOMAIN, "region outside its image");
			return -1;
		}
		if (!on_elements(r)) {
			error(MAPIM_DOMAIN, "rows must start on whole elements");
			return -1;
		}
	}
	return 0;
}

} // namespace

extern "C" {

void vips_hip_mapim_defaults(VipsHipMapim *args)
{
	if (!args)
		return;
	memset(args, 0, sizeof(*args));
	args->interpolate = VIPS_HIP_INTERPOLATE_BILINEAR;
	args->extend = VIPS_HIP_EXTEND_BACKGROUND;
	args->n_background = 1;
}

int vips_hip_mapim_bounds_need(const double bounds[4], const VipsHipMapim *args, int in_width, int in_height, int need[4])
{
	if (need)
		need[0] = need[1] = need[2] = need[3] = 0;
	if (!bounds || !args || !need || in_width < 1 || in_height < 1) {
		error(MAPIM_DOMAIN, "bad arguments");
		return -1;
	}
	if (check_args(args, VIPS_HIP_FORMAT_UCHAR))
		return -1;
	// no number in a component: every pel of the rect is ink
	if (!(bounds[0] <= bounds[2]) || !(bounds[1] <= bounds[3]))
		return 0;
	ResamplePels pels;
	const double zero = 0.0;
	if (resample_pels(MAPIM_DOMAIN, args->interpolate, args->extend, 1, 1, &zero, 1, VIPS_HIP_FORMAT_UCHAR, 0, &pels))
		return -1;
	// mapim.c:207-223: the bounding box, left and top rounded down, right and bottom up, clipped down to ints
	const double min_x = clip_coord(floor(bounds[0])), min_y = clip_coord(floor(bounds[1]));
	const double max_x = clip_coord(ceil(bounds[2])), max_y = clip_coord(ceil(bounds[3]));
	const int b_left = (int) min_x, b_top = (int) min_y;
	const int b_width = (int) ((max_x - min_x) + 1), b_height = (int) ((max_y - min_y) + 1);
	// mapim.c:351-365: the stencil, the antialias edge, the clip against the embedded image
	const long long ew = (long long) in_width + pels.window_size - 1 + 2, eh = (long long) in_height + pels.window_size - 1 + 2;
	const long long x0 = b_left + 1, y0 = b_top + 1; // (never negative)
	long long x1 = x0 + b_width + pels.window_size - 1, y1 = y0 + b_height + pels.window_size - 1;
	x1 = x1 < ew ? x1 : ew;
	y1 = y1 < eh ? y1 : eh;
	if (x1 <= x0 || y1 <= y0)
		return 0;
	// ... and as pels of the image itself, the way vips_hip_affine_need reports it
	const int off = pels.window_offset + 1;
	int px0, px1, py0, py1;
	embedded_axis_to_image(args->extend, off, in_width, (int) x0, (int) x1 - 1, &px0, &px1);
	embedded_axis_to_image(args->extend, off, in_height, (int) y0, (int) y1 - 1, &py0, &py1);
	need[0] = px0;
	need[1] = py0;
	need[2] = px1 - px0 + 1;
	need[3] = py1 - py0 + 1;
	return 0;
}

int vips_hip_mapim_need(const VipsHipRegion *index_region, const VipsHipMapim *args, int in_width, int in_height, int need[4])
{
	if (need)
		need[0] = need[1] = need[2] = need[3] = 0;
	if (!index_region || !args || !need || in_width < 1 || in_height < 1) {
		error(MAPIM_DOMAIN, "bad arguments");
		return -1;
	}
	if (ensure_init())
		return -1;
	if (check_region(MAPIM_DOMAIN, index_region) || check_index(index_region->bands, index_region->format) ||
		check_args(args, VIPS_HIP_FORMAT_UCHAR))
		return -1;
	if (!on_elements(index_region)) {
		error(MAPIM_DOMAIN, "rows must start on whole elements");
		return -1;
	}
	DeviceBlock block(4 * sizeof(int));
	if (!block.p)
		return -1;
	int found[4];
	if (mapim_bounds_run(MAPIM_DOMAIN, (const unsigned char *) index_region->data, (long long) index_region->stride, index_region->width,
			index_region->height, index_region->format, (int *) block.p) ||
		vips_hip_memcpy_d2h(found, block.p, sizeof(found)))
		return -1;
	// (already floored, ceiled and clipped: the host half does nothing to whole numbers in range)
	const double bounds[4] = { (double) found[0], (double) found[1], (double) found[2], (double) found[3] };
	return vips_hip_mapim_bounds_need(bounds, args, in_width, in_height, need);
}

int vips_hip_mapim_gen(const VipsHipRegion *in_region, const VipsHipRegion *index_region, const VipsHipRegion *out_region,
	const VipsHipMapim *args, int in_width, int in_height)
{
	if (!in_region || !index_region || !out_region || !args) {
		error(MAPIM_DOMAIN, "null argument");
		return -1;
	}
	if (ensure_init())
		return -1;
	if (check_regions(in_region, index_region, out_region, in_width, in_height) || check_index(index_region->bands, index_region->format) ||
		check_args(args, in_region->format))
		return -1;
	// the regions' image as it is: no chain, and the white of an image without an interpretation
	ResamplePels pels;
	if (resample_pels(MAPIM_DOMAIN, args->interpolate, args->extend, 1, args->n_background, args->background, in_region->bands, in_region->format,
			VIPS_HIP_INTERPRETATION_MULTIBAND, &pels))
		return -1;
	return gen_checked(in_region, index_region, out_region, args, pels, in_width, in_height);
}

// vips_mapim_build, mapim.c:430-537
int vips_hip_mapim(VipsHipImage *in, VipsHipImage *index, VipsHipImage **out, const VipsHipMapim *args)
{
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !index || !out || !args) {
		error(MAPIM_DOMAIN, "null argument");
		return -1;
	}
	if (index->device != in->device) {
		error(MAPIM_DOMAIN, "the images are on different devices");
		return -1;
	}
	if (check_index(index->bands, index->format) || check_args(args, in->format))
		return -1;
	ResamplePels pels;
	if (resample_pels(MAPIM_DOMAIN, args->interpolate, args->extend, args->premultiplied, args->n_background, args->background, in->bands,
			in->format, in->interpretation, &pels))
		return -1;
	// mapim.c:482-498: the embed comes first, so its fill pel is premultiplied with the image
	ImageRef pre;
	VipsHipImage *src = in;
	if (pels.chain) {
		if (vips_hip_premultiply(in, &pre.im, 0) || resample_fill_premultiply(MAPIM_DOMAIN, &pels, in->bands, in->format, in->interpretation))
			return -1;
		src = pre.im;
		if (src->format != pels.kformat) {
			error(MAPIM_DOMAIN, "premultiply did not make a float image");
			return -1;
		}
	}
	ImageRef o(vips_hip_image_new(index->width, index->height, in->bands, pels.kformat, in->interpretation));
	if (!o.im)
		return -1;
	VipsHipRegion ri, rx, ro;
	vips_hip_image_region(src, &ri);
	vips_hip_image_region(index, &rx);
	vips_hip_image_region(o.im, &ro);
	if (check_regions(&ri, &rx, &ro, in->width, in->height) || gen_checked(&ri, &rx, &ro, args, pels, in->width, in->height))
		return -1;
	if (pels.chain) {
		// mapim.c:526-531
		ImageRef un, back;
		if (vips_hip_unpremultiply(o.im, &un.im, 0) || vips_hip_cast(un.im, &back.im, in->format))
			return -1;
		*out = back.release();
		return 0;
	}
	*out = o.release();
	return 0;
}

int vips_hip_mapim_step(int what)
{
	return mapim_tile(what);
}

// vips_xyz_build, create/xyz.c:105-160, without csize / dsize / esize
int vips_hip_xyz(VipsHipImage **out, int width, int height)
{
	const char *domain = "xyz";
	if (!out) {
		error(domain, "null argument");
		return -1;
	}
	if (width < 1 || height < 1) {
		error(domain, "parameter %s not set", width < 1 ? "width" : "height");
		return -1;
	}
	ImageRef o(vips_hip_image_new(width, height, 2, VIPS_HIP_FORMAT_UINT, VIPS_HIP_INTERPRETATION_MULTIBAND));
	if (!o.im)
		return -1;
	if (xyz_run(domain, (unsigned char *) o.im->data, (long long) o.im->stride, width, height))
		return -1;
	*out = o.release();
	return 0;
}

} // extern "C"
