// vips_rank / vips_median (morphology/rank.c) and vips_morph (morphology/morph.c) on images in HBM: the host side --
// the reference's argument checks with its messages, the region checks, the C ABI.  The kernels are rank.hip and
// morph.hip.
#include "internal.h"

#include <cmath>
#include <vector>

using namespace vh;

// The checks every neighbourhood gen makes on its pair of regions, and the geometry of the launch: @in must hold the
// out rect grown by the window (origin win_w / 2, win_h / 2) and clipped to the image.
int vh::nb_geometry(const char *domain, const VipsHipRegion *in, const VipsHipRegion *out, int win_w, int win_h, NbArgs *a)
{
	if (in->bands != out->bands) {
		error(domain, "output region has the wrong bands");
		return -1;
	}
	if (in->im_width != out->im_width || in->im_height != out->im_height) {
		error(domain, "input and output images must have the same size");
		return -1;
	}
	if (in->left < 0 || in->top < 0 || (long long) in->left + in->width > in->im_width || (long long) in->top + in->height > in->im_height ||
		out->left < 0 || out->top < 0 || (long long) out->left + out->width > out->im_width ||
		(long long) out->top + out->height > out->im_height) {
		error(domain, "region outside its image");
		return -1;
	}
	int x0 = out->left - win_w / 2, x1 = out->left + out->width - 1 - win_w / 2 + win_w - 1;
	int y0 = out->top - win_h / 2, y1 = out->top + out->height - 1 - win_h / 2 + win_h - 1;
	x0 = x0 < 0 ? 0 : x0;
	y0 = y0 < 0 ? 0 : y0;
	x1 = x1 > in->im_width - 1 ? in->im_width - 1 : x1;
	y1 = y1 > in->im_height - 1 ? in->im_height - 1 : y1;
	if (x0 < in->left || y0 < in->top || x1 >= in->left + in->width || y1 >= in->top + in->height) {
		error(domain, "input region too small");
		return -1;
	}
	// element indexes are ints in the kernels; rows of blocks go in the grid's y
	if (((long long) in->im_width + win_w) * in->bands * format_sizeof(in->format) >= (1LL << 31) ||
		out->height > 65535 * 8) {
		error(domain, "image too large");
		return -1;
	}
	a->in = (const unsigned char *) in->data;
	a->out = (unsigned char *) out->data;
	a->in_stride = (long long) in->stride;
	a->out_stride = (long long) out->stride;
	a->in_left = in->left;
	a->in_top = in->top;
	a->in_width = in->width;
	a->in_height = in->height;
	a->im_width = in->im_width;
	a->im_height = in->im_height;
	a->out_left = out->left;
	a->out_top = out->top;
	a->out_width = out->width;
	a->out_height = out->height;
	a->bands = in->bands;
	a->win_w = win_w;
	a->win_h = win_h;
	a->lds_row = 0;
	a->index = 0;
	a->key_xor = 0;
	return 0;
}

extern "C" {

// vips_rank_generate, rank.c:412-456, with the checks of vips_rank_build :477-489 (on the whole image's size)
int vips_hip_rank_gen(const VipsHipRegion *in, const VipsHipRegion *out, int width, int height, int index)
{
	const char *domain = "rank";
	if (ensure_init())
		return -1;
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (format_iscomplex(in->format)) {
		error(domain, "image must be non-complex");
		return -1;
	}
	if (width < 1 || height < 1 || width > in->im_width || height > in->im_height) {
		error(domain, "window too large");
		return -1;
	}
	if (index < 0 || (long long) index > (long long) width * height - 1) {
		error(domain, "index out of range");
		return -1;
	}
	if (in->format == VIPS_HIP_FORMAT_DOUBLE) {
		error(domain, "double images are outside the HIP path");
		return -1;
	}
	if (out->format != in->format) {
		error(domain, "output region has the wrong format");
		return -1;
	}
	NbArgs a;
	if (nb_geometry(domain, in, out, width, height, &a))
		return -1;
	a.index = index;
	return rank_run(domain, a, in->format);
}

// vips_dilate_gen / vips_erode_gen, morph.c:662-826, with the mask checks of vips_morph_build :872-892
int vips_hip_morph_gen(const VipsHipRegion *in, const VipsHipRegion *out, const double *mask, int mask_width, int mask_height,
	int morph)
{
	const char *domain = "morph";
	if (ensure_init())
		return -1;
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (!mask || mask_width < 1 || mask_height < 1) {
		error(domain, "bad mask");
		return -1;
	}
	if (morph != 0 && morph != 1) {
		error(domain, "morph should be 0 (erode) or 1 (dilate)");
		return -1;
	}
	if (format_iscomplex(in->format)) {
		error(domain, "complex images are outside the HIP path");
		return -1;
	}
	if (out->format != VIPS_HIP_FORMAT_UCHAR) {
		error(domain, "the output is uchar");
		return -1;
	}
	if (mask_width > morph_tile(2) || mask_height > morph_tile(2)) {
		error(domain, "a %d x %d mask: the kernel takes masks up to %d x %d", mask_width, mask_height, morph_tile(2), morph_tile(2));
		return -1;
	}
	// vips__image_intize rint()s every element (convi.c:892-895), then morph.c:882-891
	std::vector<unsigned char> coeff((size_t) mask_width * mask_height);
	for (size_t i = 0; i < coeff.size(); i++) {
		const double v = rint(mask[i]);
		if (v != 0 && v != 128 && v != 255) {
			error(domain, "bad mask element (%f should be 0, 128 or 255)", v);
			return -1;
		}
		coeff[i] = (unsigned char) (int) v;
	}
	NbArgs a;
	if (nb_geometry(domain, in, out, mask_width, mask_height, &a))
		return -1;
	if (in->format == VIPS_HIP_FORMAT_UCHAR)
		return morph_run(domain, a, coeff.data(), morph);
	// "Make sure we are uchar" (morph.c:866-870): vips_cast of the window, then the kernel on the cast rows.  (The
	// block goes back to the pool behind the kernel: the pool hands it out again on this thread's stream only.)
	VipsHipRegion cast = *in;
	cast.format = VIPS_HIP_FORMAT_UCHAR;
	cast.stride = (size_t) in->width * in->bands;
	DeviceBlock block(cast.stride * in->height);
	if (!block.p)
		return -1;
	cast.data = block.p;
	if (vips_hip_cast_gen(in, &cast))
		return -1;
	a.in = (const unsigned char *) cast.data;
	a.in_stride = (long long) cast.stride;
	return morph_run(domain, a, coeff.data(), morph);
}

void vips_hip_rank_need(int window_height, int top, int height, int *in_top, int *in_height)
{
	if (in_top)
		*in_top = top - window_height / 2;
	if (in_height)
		*in_height = height + window_height - 1;
}

int vips_hip_rank_step(int what)
{
	switch (what) {
	case 0:
	case 1:
		return rank_tile(what);
	case 2:
	case 3:
	case 4:
		return morph_tile(what - 2);
	default:
		return 0;
	}
}

// vips_rank_build, rank.c:458-539
int vips_hip_rank(VipsHipImage *in, VipsHipImage **out, int width, int height, int index)
{
	if (enter("rank", in, out))
		return -1;
	return whole_image(in, out, in->bands, in->format,
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_rank_gen(ri, ro, width, height, index); });
}

// vips_median, rank.c:639-671
int vips_hip_median(VipsHipImage *in, VipsHipImage **out, int size)
{
	if (size < 1 || size > 46340) {
		error("rank", "window too large");
		return -1;
	}
	return vips_hip_rank(in, out, size, size, size * size / 2);
}

// vips_morph_build, morph.c:828-941
int vips_hip_morph(VipsHipImage *in, VipsHipImage **out, const double *mask, int mask_width, int mask_height, int morph)
{
	if (enter("morph", in, out))
		return -1;
	return whole_image(in, out, in->bands, VIPS_HIP_FORMAT_UCHAR,
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_morph_gen(ri, ro, mask, mask_width, mask_height, morph); });
}

} // extern "C"
