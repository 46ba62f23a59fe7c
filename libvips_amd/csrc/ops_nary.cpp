// vips_sum (arithmetic/sum.c) and vips_bandrank (conversion/bandrank.c) on images in HBM: the host side -- each build()
// restated (vips__formatalike_vec, vips__bandalike_vec and vips__sizealike_vec over the array, sum's format table,
// bandrank's index rule and its copy of one image, the errors with the reference's words), the C ABI.  The kernels are
// in nary.hip.
#include "internal.h"

#include <cstring>

using namespace vh;

static_assert(NARY_IMAGES == VIPS_HIP_BANDJOIN_MAX, "one length for an array of images");

namespace {

const char *const NICKNAMES[2] = { "sum", "bandrank" };

// the common header of the array, or the refusal; *op the kernel's operation
int plan_images(int rank, VipsHipImage **in, int n, int index, int *format, int *out_format, int *bands, int *interpretation,
	int *width, int *height, int *out_index)
{
	int widths[NARY_IMAGES], heights[NARY_IMAGES], nbands[NARY_IMAGES], formats[NARY_IMAGES], interps[NARY_IMAGES];
	for (int i = 0; i < n; i++) {
		widths[i] = in[i]->width;
		heights[i] = in[i]->height;
		nbands[i] = in[i]->bands;
		formats[i] = in[i]->format;
		interps[i] = in[i]->interpretation;
	}
	return vips_hip_nary_plan(rank, n, widths, heights, nbands, formats, interps, index, format, out_format, bands, interpretation,
		width, height, out_index);
}

int nary_image(int rank, VipsHipImage **in, int n, VipsHipImage **out, int index)
{
	const char *domain = NICKNAMES[rank];
	if (!in || !out || n < 1 || !in[0]) {
		error(domain, n < 1 && in && out ? "no input images" : "null argument");
		return -1;
	}
	if (bind_to(in[0]))
		return -1;
	if (n > NARY_IMAGES) {
		error(domain, "arrays of more than %d images are outside the HIP path", NARY_IMAGES);
		return -1;
	}
	for (int i = 0; i < n; i++) {
		if (!in[i]) {
			error(domain, "null argument");
			return -1;
		}
		if (in[i]->device != in[0]->device) {
			error(domain, "the images are on different devices");
			return -1;
		}
	}
	int format, out_format, bands, interpretation, width, height, rank_index;
	if (plan_images(rank, in, n, index, &format, &out_format, &bands, &interpretation, &width, &height, &rank_index))
		return -1;
	// bandrank.c:211-216: one image is a copy
	if (rank && n == 1)
		return vips_hip_cast(in[0], out, in[0]->format);
	ImageRef cast[NARY_IMAGES];
	ImageRef o(vips_hip_image_new(width, height, bands, out_format, interpretation));
	if (!o.im)
		return -1;
	NaryArgs a;
	memset(&a, 0, sizeof(a));
	a.out = (unsigned char *) o.im->data;
	a.out_stride = (long long) o.im->stride;
	a.elems = width * bands;
	a.height = height;
	a.bands = bands;
	a.n = n;
	a.index = rank_index;
	for (int i = 0; i < n; i++) {
		// vips__formatalike_vec: vips_cast of what is not in the common format
		VipsHipImage *im = in[i];
		if (im->format != format) {
			if (vips_hip_cast(im, &cast[i].im, format))
				return -1;
			im = cast[i].im;
		}
		a.src[i].in = (const unsigned char *) im->data;
		a.src[i].stride = (long long) im->stride;
		a.src[i].width = im->width;
		a.src[i].height = im->height;
		a.src[i].bands = im->bands;
	}
	const int op = !rank ? NARY_SUM : rank_index == 0 ? NARY_MIN : rank_index == n - 1 ? NARY_MAX : NARY_RANK;
	if (nary_run(domain, op, format, a))
		return -1;
	*out = o.release();
	return 0;
}

} // namespace

extern "C" {

int vips_hip_nary_plan(int rank, int n, const int *widths, const int *heights, const int *bands, const int *formats,
	const int *interpretations, int index, int *format, int *out_format, int *out_bands, int *interpretation, int *width,
	int *height, int *out_index)
{
	const char *domain = NICKNAMES[rank ? 1 : 0];
	if (!widths || !heights || !bands || !formats || !interpretations || !format || !out_format || !out_bands || !interpretation ||
		!width || !height) {
		error(domain, "null argument");
		return -1;
	}
	if (n < 1) {
		error(domain, "no input images");
		return -1;
	}
	if (n > NARY_IMAGES) {
		error(domain, "arrays of more than %d images are outside the HIP path", NARY_IMAGES);
		return -1;
	}
	*width = *height = 0;
	for (int i = 0; i < n; i++) {
		if (widths[i] < 1 || heights[i] < 1 || bands[i] < 1) {
			error(domain, "bad image size");
			return -1;
		}
		// bandrank.c:207-209; sum's table has no real format for a complex one, which stays out as everywhere in the family
		if (arithmetic_noncomplex(domain, formats[i]))
			return -1;
		*format = i ? format_common(*format, formats[i]) : formats[0];
		*width = widths[i] > *width ? widths[i] : *width;
		*height = heights[i] > *height ? heights[i] : *height;
	}
	if (bandalike(domain, bands, interpretations, n, out_bands, interpretation))
		return -1;
	int at = index;
	if (rank && n > 1) {
		// bandrank.c:225-230
		if (index == -1)
			at = n / 2;
		else if (index >= n || index < -1) {
			error(domain, "index out of range");
			return -1;
		}
	}
	if (out_index)
		*out_index = rank ? at : 0;
	// sum.c:137-140: uint for the unsigned formats, int for the signed ones; bandrank keeps the common format
	static const int sum_table[10] = { VIPS_HIP_FORMAT_UINT, VIPS_HIP_FORMAT_INT, VIPS_HIP_FORMAT_UINT, VIPS_HIP_FORMAT_INT,
		VIPS_HIP_FORMAT_UINT, VIPS_HIP_FORMAT_INT, VIPS_HIP_FORMAT_FLOAT, VIPS_HIP_FORMAT_COMPLEX, VIPS_HIP_FORMAT_DOUBLE,
		VIPS_HIP_FORMAT_DPCOMPLEX };
	*out_format = rank ? *format : sum_table[*format];
	if ((long long) *width * *out_bands >= (1LL << 31) / 8) {
		error(domain, "image rows too long");
		return -1;
	}
	return 0;
}

int vips_hip_sum(VipsHipImage **in, int n, VipsHipImage **out)
{
	return nary_image(0, in, n, out, 0);
}

int vips_hip_bandrank(VipsHipImage **in, int n, VipsHipImage **out, int index)
{
	return nary_image(1, in, n, out, index);
}

int vips_hip_nary_step(int what)
{
	return nary_tile(what);
}

} // extern "C"
