// vips_labelregions and vips_countlines (morphology/labelregions.c, countlines.c) on images in HBM: the host side -- the
// checks and refusals, the mask's header, the planes from the pool, countlines' finish in the reference's order, the C
// ABI.  The kernels are in regions.hip.
#include "internal.h"

using namespace vh;

namespace {

// what both operations ask of the input: a real format, rows that start on whole elements
int check_real(const char *domain, const VipsHipImage *in)
{
	if (format_iscomplex(in->format) || format_sizeof(in->format) == 0) {
		error(domain, "complex images are outside the HIP path");
		return -1;
	}
	if (in->width < 1 || in->height < 1 || in->bands < 1) {
		error(domain, "bad image");
		return -1;
	}
	if (((uintptr_t) in->data | (uintptr_t) in->stride) % (uintptr_t) format_sizeof(in->format)) {
		error(domain, "rows must start on whole elements");
		return -1;
	}
	return 0;
}

} // namespace

extern "C" {

int vips_hip_labelregions(VipsHipImage *in, VipsHipImage **mask, int *segments)
{
	const char *domain = "labelregions";
	if (enter(domain, in, mask))
		return -1;
	if (check_real(domain, in))
		return -1;
	if ((long long) in->bands * format_sizeof(in->format) > REGIONS_MAX_PEL) {
		error(domain, "pels of more than %d bytes are outside the HIP path", REGIONS_MAX_PEL);
		return -1;
	}
	// a label is an int, and so is a pel's linear index
	if ((long long) in->width * in->height >= (1LL << 31)) {
		error(domain, "images of 2^31 pels and more are outside the HIP path (%d x %d)", in->width, in->height);
		return -1;
	}
	RegionsLayout l;
	regions_layout(in->width, in->height, &l);
	// vips_black cast to int (labelregions.c:76-78): one band, multiband.  No strips: a region can span the image, so
	// the mask and the planes lie in HBM whole or the call is refused
	const size_t mask_bytes = (size_t) in->width * in->height * sizeof(int);
	ImageRef o(vips_hip_image_new(in->width, in->height, 1, VIPS_HIP_FORMAT_INT, VIPS_HIP_INTERPRETATION_MULTIBAND));
	DeviceBlock planes(o.im ? l.bytes : 0);
	if (!o.im || !planes.p) {
		error(domain, "a %d x %d image takes a mask of %zu bytes and planes of %zu bytes in device memory, whole: there are no strips",
			in->width, in->height, mask_bytes, l.bytes);
		return -1;
	}
	if (regions_label_run(domain, in, (unsigned char *) planes.p, (int *) o.im->data))
		return -1;
	if (segments) {
		// the call's only download.  labelregions.c:86, :97, :104-106: the counter starts at 1 and is stored after the
		// last increment
		int regions = 0;
		if (vips_hip_memcpy_d2h(&regions, (unsigned char *) planes.p + l.total, sizeof(int)))
			return -1;
		*segments = regions + 1;
	}
	*mask = o.release();
	return 0;
}

int vips_hip_labelregions_step(int what)
{
	return what >= 0 && what <= 2 ? regions_tile(what) : 0;
}

int vips_hip_countlines(VipsHipImage *in, int direction, double *nolines)
{
	const char *domain = "countlines";
	if (enter(domain, in, nolines))
		return -1;
	if (direction != 0 && direction != 1) {
		error(domain, "enum 'VipsDirection' has no member %d", direction);
		return -1;
	}
	if (check_real(domain, in))
		return -1;
	if ((long long) in->width * in->bands >= (1LL << 31)) {
		error(domain, "image too large");
		return -1;
	}
	// the reference's sums are project's guint (project.c:99-102): 255 a rise, at most every other pel one.  Past 2^25
	// pels along the direction a sum could wrap, and the wrapped average is not what this path computes
	const int along = direction == 0 ? in->height : in->width;
	if (along > (1 << 25)) {
		error(domain, "images of more than %d pels along the count are outside the HIP path", 1 << 25);
		return -1;
	}
	DeviceBlock rises(sizeof(unsigned long long));
	if (!rises.p)
		return -1;
	VH_CHECK(hipMemsetAsync(rises.p, 0, sizeof(unsigned long long), stream()));
	if (countlines_run(domain, in, direction, (unsigned long long *) rises.p))
		return -1;
	unsigned long long total = 0;
	if (vips_hip_memcpy_d2h(&total, rises.p, sizeof(total)))
		return -1;
	// countlines.c:98-99 / :109-110, :118: vips_avg of the projection across the direction -- its uint sums, 255 a rise,
	// added in double (avg.c: exact in any order below 2^53) and divided by the number of values, extent x bands -- then
	// / 255.0
	const double sum = 255.0 * (double) total;
	const double vals = (double) ((unsigned long long) (direction == 0 ? in->width : in->height) * (unsigned long long) in->bands);
	*nolines = sum / vals / 255.0;
	return 0;
}

} // extern "C"
