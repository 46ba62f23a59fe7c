// vips_rot, vips_flip and vips_autorot on images in HBM, and the orientation accessors: the host side.  The kernel is
// rot.hip.
#include "internal.h"

using namespace vh;

extern "C" {

// vips_rot, conversion/rot.c:349-400; vips_flip, conversion/flip.c:230-262; vips_autorot, conversion/autorot.c:103-191
static int rot_image(const char *domain, VipsHipImage *in, VipsHipImage **out, int op, int orientation)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (op == 0) { // vips_copy: the same pixels
		VipsHipImage *shared = image_share(in);
		if (!shared) {
			ImageRef c(vips_hip_image_new(in->width, in->height, in->bands, in->format, in->interpretation));
			if (!c.im || vips_hip_memcpy_d2d(c.im->data, in->data, in->stride * in->height))
				return -1;
			shared = c.release();
		}
		shared->orientation = orientation;
		*out = shared;
		return 0;
	}
	const bool transpose = (op & vh::ROT_OP_TRANSPOSE) != 0;
	ImageRef o(vips_hip_image_new(transpose ? in->height : in->width, transpose ? in->width : in->height, in->bands,
		in->format, in->interpretation));
	if (!o.im)
		return -1;
	VipsHipRegion ri, ro;
	vips_hip_image_region(in, &ri);
	vips_hip_image_region(o.im, &ro);
	if (vh::rot_op_gen(domain, op, &ri, &ro))
		return -1;
	o.im->orientation = orientation;
	*out = o.release();
	return 0;
}

int vips_hip_rot(VipsHipImage *in, VipsHipImage **out, int angle)
{
	static const int ops[4] = { 0, vh::ROT_OP_TRANSPOSE | vh::ROT_OP_FLIPY, vh::ROT_OP_FLIPX | vh::ROT_OP_FLIPY,
		vh::ROT_OP_TRANSPOSE | vh::ROT_OP_FLIPX };
	if (angle < 0 || angle > 3) {
		error("rot", "bad angle %d", angle);
		return -1;
	}
	return rot_image("rot", in, out, ops[angle], in ? in->orientation : 0);
}

int vips_hip_flip(VipsHipImage *in, VipsHipImage **out, int direction)
{
	if (direction != 0 && direction != 1) {
		error("flip", "bad direction %d", direction);
		return -1;
	}
	return rot_image("flip", in, out, direction == 0 ? vh::ROT_OP_FLIPX : vh::ROT_OP_FLIPY, in ? in->orientation : 0);
}

int vips_hip_autorot(VipsHipImage *in, VipsHipImage **out, int *angle, int *flip)
{
	if (!in || !out) {
		error("autorot", "null argument");
		return -1;
	}
	// autorot.c:119-160
	static const int angles[9] = { 0, 0, 0, 2, 2, 1, 1, 3, 3 };
	static const int flips[9] = { 0, 0, 1, 0, 1, 1, 0, 1, 0 };
	const int orientation = in->orientation >= 1 && in->orientation <= 8 ? in->orientation : 1;
	if (rot_image("autorot", in, out, vh::orientation_op(orientation), 0))
		return -1;
	if (angle)
		*angle = angles[orientation];
	if (flip)
		*flip = flips[orientation];
	return 0;
}

int vips_hip_image_get_orientation(const VipsHipImage *image)
{
	return image && image->orientation >= 1 && image->orientation <= 8 ? image->orientation : 0;
}

int vips_hip_image_set_orientation(VipsHipImage *image, int orientation)
{
	if (!image) {
		error("VipsImage", "null argument");
		return -1;
	}
	if (orientation < 0 || orientation > 8) {
		error("VipsImage", "orientation %d is not 0 (none) or 1 .. 8", orientation);
		return -1;
	}
	image->orientation = orientation;
	return 0;
}

} // extern "C"
