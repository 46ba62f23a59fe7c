// vips_extract_area and vips_thumbnail_image on images in HBM: the host side -- thumbnail.c's pipeline (processing
// space, shrink, premultiply round the resize, back to the output space, auto-rotation, crop) over the library's own
// operations, the C ABI.
#include "colour.h"
#include "reduce_u8.h"

using namespace vh;

extern "C" {

// vips_extract_area (conversion/extract.c:137-187): a rectangle of the image, as a new image
int vips_hip_extract_area(VipsHipImage *in, VipsHipImage **out, int left, int top, int width, int height)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error("extract_area", "null argument");
		return -1;
	}
	if (width <= 0 || height <= 0 || left < 0 || top < 0 || (long long) left + width > in->width ||
		(long long) top + height > in->height) {
		error("extract_area", "bad extract area");
		return -1;
	}
	ImageRef o(vips_hip_image_new(width, height, in->bands, in->format, in->interpretation));
	if (!o.im)
		return -1;
	const size_t pel = (size_t) in->bands * format_sizeof(in->format);
	const unsigned char *src = (const unsigned char *) in->data + (size_t) top * in->stride + (size_t) left * pel;
	if (hipMemcpy2DAsync(o.im->data, o.im->stride, src, in->stride, (size_t) width * pel, (size_t) height,
			hipMemcpyDeviceToDevice, stream()) != hipSuccess) {
		error("extract_area", "device copy failed");
		return -1;
	}
	*out = o.release();
	return 0;
}

// vips_thumbnail_build, resample/thumbnail.c:678-1067, for in-memory images
// (vips_thumbnail_image: no pre-shrink on load, no pages).
int vips_hip_thumbnail_image(VipsHipImage *in, VipsHipImage **out, int width, int height, int size,
	int linear)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	return vips_hip_thumbnail_image_crop(in, out, width, height, size, linear, 0);
}

// ... with the crop argument: a VipsInteresting (include/vips/conversion.h:97-107), which vips_hip_smartcrop
// (smartcrop.cpp) carries out on the finished thumbnail: the positional modes (none 0, centre 1, low 4, high 5,
// all 6) and the content-driven ones (entropy 2, attention 3) for the images it takes.
//
// @rotate: the orientation vips_autorot undoes between the conversion back to the output space and the crop
// (thumbnail.c:989-1062), 0 or 1 for none.  One that swaps the axes (5 .. 8) swaps the target box for the shrink
// calculation (thumbnail.c:416-420), so that the crop works on the upright image with the box as given.
static int thumbnail_image_any(VipsHipImage *in, VipsHipImage **out, int width, int height, int size, int linear,
	int crop, int rotate)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	const char *domain = "thumbnail";
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (crop < 0 || crop > 6) {
		error(domain, "bad crop mode %d", crop);
		return -1;
	}
	// what vips_hip_smartcrop would refuse at the end whatever the pipeline does (the band count stays): now,
	// before any kernel runs
	if ((crop == 2 || crop == 3) && (in->bands == 2 || in->bands > 3)) {
		error(domain, "crop mode '%s' does not take images with alpha", crop == 2 ? "entropy" : "attention");
		return -1;
	}
	if (crop == 3 && in->bands < 3) {
		error(domain, "crop mode 'attention' takes 3-band images (no B_W to XYZ route)");
		return -1;
	}
	if (width <= 0) {
		error(domain, "parameter width not set");
		return -1;
	}
	if (height <= 0)
		height = width; // thumbnail.c:720-721
	if (size < 0 || size > 3) {
		error(domain, "bad size mode %d", size);
		return -1;
	}

	// processing space (thumbnail.c:763-823)
	ImageRef space;
	VipsHipImage *cur;
	{
		// sRGB or, with fewer than 3 bands, B_W; linear: scRGB or GREY16 (thumbnail.c:791-822).
		// Already there (the usual sRGB uchar photograph, a greyscale JPEG): vips_colourspace is a pointer copy then,
		// and this function only reads the result -- caller-owned device memory, which vips_hip_colourspace would have
		// to copy to own, is read where it is
		const int target = in->bands < 3 ? (linear ? VIPS_HIP_INTERPRETATION_GREY16 : VIPS_HIP_INTERPRETATION_B_W)
										 : (linear ? VIPS_HIP_INTERPRETATION_scRGB : VIPS_HIP_INTERPRETATION_sRGB);
		const Route *route = route_find(image_guess_interpretation(in), target);
		if (route && route->n == 0 && route->cast_format == in->format)
			cur = in;
		else {
			if (vips_hip_colourspace(in, &space.im, target))
				return -1;
			cur = space.im;
		}
	}

	// vips_thumbnail_calculate_shrink, thumbnail.c:413-467
	const bool swap = rotate >= 5 && rotate <= 8;
	double hshrink = (double) cur->width / (swap ? height : width);
	double vshrink = (double) cur->height / (swap ? width : height);
	// fit the box (the bigger shrink wins) or, when cropping, fill it (the smaller one)
	const bool horizontal = crop != 0 ? (hshrink < vshrink) : !(hshrink < vshrink);
	if (size != 3) { // != VIPS_SIZE_FORCE
		if (horizontal)
			vshrink = hshrink;
		else
			hshrink = vshrink;
	}
	if (size == 1) { // VIPS_SIZE_UP
		hshrink = hshrink < 1 ? hshrink : 1;
		vshrink = vshrink < 1 ? vshrink : 1;
	}
	else if (size == 2) { // VIPS_SIZE_DOWN
		hshrink = hshrink > 1 ? hshrink : 1;
		vshrink = vshrink > 1 ? vshrink : 1;
	}
	hshrink = hshrink < cur->width ? hshrink : cur->width;
	vshrink = vshrink < cur->height ? vshrink : cur->height;

	// vips_image_hasalpha: premultiply before shrinking (thumbnail.c:848-860), staying in
	// uchar when the image is uchar
	int unpremultiplied_format = -1;
	ImageRef pre;
	ImageRef resized;
	if ((cur->bands == 2 || cur->bands > 3) && hshrink != 1.0 && vshrink != 1.0) {
		unpremultiplied_format = cur->format;
		// RGBA uchar with 8-bit alpha: the premultiply on the loads of the resize's first kernel (no premultiplied
		// image in between: 268 MB written and read again for an 8192 x 8192 input) when the chain of band kernels
		// takes the resize; else the operation, then the resize
		if (cur->format == VIPS_HIP_FORMAT_UCHAR && cur->bands == 4 && interpretation_max_alpha(cur->interpretation) == 255.0) {
			const int r = vh::resize_premul_u8(cur, &resized.im, 1.0 / hshrink, 1.0 / vshrink);
			if (r < 0)
				return -1;
		}
		if (!resized.im) {
			if (vips_hip_premultiply(cur, &pre.im, cur->format == VIPS_HIP_FORMAT_UCHAR))
				return -1;
			cur = pre.im;
		}
	}

	if (!resized.im && vips_hip_resize(cur, &resized.im, 1.0 / hshrink, 1.0 / vshrink, VIPS_HIP_KERNEL_LANCZOS3, 2.0))
		return -1;

	if (unpremultiplied_format >= 0) { // thumbnail.c:886-904
		ImageRef un;
		if (unpremultiplied_format == VIPS_HIP_FORMAT_UCHAR) {
			if (vips_hip_unpremultiply(resized.im, &un.im, 1))
				return -1;
		}
		else {
			ImageRef f;
			if (vips_hip_unpremultiply(resized.im, &f.im, 0) ||
				vips_hip_cast(f.im, &un.im, unpremultiplied_format))
				return -1;
		}
		vips_hip_image_unref(resized.im);
		resized.im = un.release();
	}

	if (linear) { // thumbnail.c:973-987: back to sRGB, or to B_W with fewer than 3 bands
		ImageRef back;
		if (vips_hip_colourspace(resized.im, &back.im,
				resized.im->bands < 3 ? VIPS_HIP_INTERPRETATION_B_W : VIPS_HIP_INTERPRETATION_sRGB))
			return -1;
		vips_hip_image_unref(resized.im);
		resized.im = back.release();
	}
	if (vh::orientation_op(rotate) != 0) { // thumbnail.c:989-997
		resized.im->orientation = rotate;
		ImageRef upright;
		if (vips_hip_autorot(resized.im, &upright.im, nullptr, nullptr))
			return -1;
		vips_hip_image_unref(resized.im);
		resized.im = upright.release();
	}
	if (crop != 0) { // thumbnail.c:1010-1038
		const VipsHipImage *r = resized.im;
		const int crop_width = width < r->width ? width : r->width;
		const int crop_height = height < r->height ? height : r->height;
		return vips_hip_smartcrop(resized.im, out, crop_width, crop_height, crop, nullptr, nullptr, nullptr, nullptr);
	}
	*out = resized.release();
	return 0;
}

int vips_hip_thumbnail_image_crop(VipsHipImage *in, VipsHipImage **out, int width, int height, int size,
	int linear, int crop)
{
	return thumbnail_image_any(in, out, width, height, size, linear, crop, 0);
}

// ... with vips_thumbnail's auto-rotation: the image's orientation is undone (@no_rotate 0; the result has none), or
// the pixels are left as stored and the result keeps it (@no_rotate 1)
int vips_hip_thumbnail_image_rotate(VipsHipImage *in, VipsHipImage **out, int width, int height, int size,
	int linear, int crop, int no_rotate)
{
	if (!in || !out) {
		error("thumbnail", "null argument");
		return -1;
	}
	const int orientation = in->orientation;
	if (thumbnail_image_any(in, out, width, height, size, linear, crop, no_rotate ? 0 : orientation))
		return -1;
	if (no_rotate)
		(*out)->orientation = orientation; // (the result is an object of its own even where it shares pixels)
	return 0;
}

} // extern "C"
