// vips_colourspace, vips_cast, vips_premultiply and vips_unpremultiply on images in HBM: the host side -- the route
// table of colourspace.c, the casts and passes a route needs on THIS image, the C ABI.  The kernels are colour.hip
// and its parts colour_cast.h and colour_premultiply.h.
#include "colour.h"

using namespace vh;

namespace {

const char *interpretation_nick(int v)
{
	switch (v) {
	case VIPS_HIP_INTERPRETATION_MULTIBAND: return "multiband";
	case VIPS_HIP_INTERPRETATION_B_W: return "b-w";
	case VIPS_HIP_INTERPRETATION_XYZ: return "xyz";
	case VIPS_HIP_INTERPRETATION_LAB: return "lab";
	case VIPS_HIP_INTERPRETATION_LABS: return "labs";
	case VIPS_HIP_INTERPRETATION_sRGB: return "srgb";
	case VIPS_HIP_INTERPRETATION_RGB16: return "rgb16";
	case VIPS_HIP_INTERPRETATION_GREY16: return "grey16";
	case VIPS_HIP_INTERPRETATION_scRGB: return "scrgb";
	default: return "unknown";
	}
}

enum {
	S_sRGB2scRGB = VIPS_HIP_COLOUR_sRGB2scRGB,
	S_scRGB2XYZ = VIPS_HIP_COLOUR_scRGB2XYZ,
	S_XYZ2Lab = VIPS_HIP_COLOUR_XYZ2Lab,
	S_Lab2XYZ = VIPS_HIP_COLOUR_Lab2XYZ,
	S_XYZ2scRGB = VIPS_HIP_COLOUR_XYZ2scRGB,
	S_scRGB2sRGB = VIPS_HIP_COLOUR_scRGB2sRGB,
	S_Lab2LabS = VIPS_HIP_COLOUR_Lab2LabS,
	S_LabS2Lab = VIPS_HIP_COLOUR_LabS2Lab,
	S_scRGB2sRGB16 = VIPS_HIP_COLOUR_scRGB2sRGB16,
	S_scRGB2BW = VIPS_HIP_COLOUR_scRGB2BW,
	S_scRGB2BW16 = VIPS_HIP_COLOUR_scRGB2BW16,
	S_BW2sRGB = VIPS_HIP_COLOUR_BW2sRGB,
	S_GREY162RGB16 = VIPS_HIP_COLOUR_GREY162RGB16,
	S_sRGB2RGB16 = VIPS_HIP_COLOUR_sRGB2RGB16,
	S_RGB162sRGB = VIPS_HIP_COLOUR_RGB162sRGB
};

#define XYZ VIPS_HIP_INTERPRETATION_XYZ
#define LAB VIPS_HIP_INTERPRETATION_LAB
#define LABS VIPS_HIP_INTERPRETATION_LABS
#define scRGB VIPS_HIP_INTERPRETATION_scRGB
#define sRGB VIPS_HIP_INTERPRETATION_sRGB
#define BW VIPS_HIP_INTERPRETATION_B_W
#define RGB16 VIPS_HIP_INTERPRETATION_RGB16
#define GREY16 VIPS_HIP_INTERPRETATION_GREY16

// (S_sRGB2scRGB in a route that starts in B_W, GREY16 or RGB16 is vips_sRGB2scRGB as the reference calls it: 8 or
// 16 bits by the TAG of the image that enters the step, sRGB2scRGB.c:115-123 -- resolved in vips_hip_colourspace)
const Route routes[] = {
	{ XYZ, XYZ, 0, {}, VIPS_HIP_FORMAT_FLOAT },
	{ XYZ, LAB, 1, { S_XYZ2Lab }, -1 },
	{ XYZ, LABS, 2, { S_XYZ2Lab, S_Lab2LabS }, -1 },
	{ XYZ, scRGB, 1, { S_XYZ2scRGB }, -1 },
	{ XYZ, sRGB, 2, { S_XYZ2scRGB, S_scRGB2sRGB }, -1 },
	{ XYZ, BW, 2, { S_XYZ2scRGB, S_scRGB2BW }, -1 },
	{ XYZ, RGB16, 2, { S_XYZ2scRGB, S_scRGB2sRGB16 }, -1 },
	{ XYZ, GREY16, 2, { S_XYZ2scRGB, S_scRGB2BW16 }, -1 },

	{ LAB, XYZ, 1, { S_Lab2XYZ }, -1 },
	{ LAB, LAB, 0, {}, VIPS_HIP_FORMAT_FLOAT },
	{ LAB, LABS, 1, { S_Lab2LabS }, -1 },
	{ LAB, scRGB, 2, { S_Lab2XYZ, S_XYZ2scRGB }, -1 },
	{ LAB, sRGB, 3, { S_Lab2XYZ, S_XYZ2scRGB, S_scRGB2sRGB }, -1 },
	{ LAB, BW, 3, { S_Lab2XYZ, S_XYZ2scRGB, S_scRGB2BW }, -1 },
	{ LAB, RGB16, 3, { S_Lab2XYZ, S_XYZ2scRGB, S_scRGB2sRGB16 }, -1 },
	{ LAB, GREY16, 3, { S_Lab2XYZ, S_XYZ2scRGB, S_scRGB2BW16 }, -1 },

	{ LABS, XYZ, 2, { S_LabS2Lab, S_Lab2XYZ }, -1 },
	{ LABS, LAB, 1, { S_LabS2Lab }, -1 },
	{ LABS, LABS, 0, {}, VIPS_HIP_FORMAT_SHORT },
	{ LABS, scRGB, 3, { S_LabS2Lab, S_Lab2XYZ, S_XYZ2scRGB }, -1 },
	{ LABS, sRGB, 4, { S_LabS2Lab, S_Lab2XYZ, S_XYZ2scRGB, S_scRGB2sRGB }, -1 },
	{ LABS, BW, 4, { S_LabS2Lab, S_Lab2XYZ, S_XYZ2scRGB, S_scRGB2BW }, -1 },
	{ LABS, RGB16, 4, { S_LabS2Lab, S_Lab2XYZ, S_XYZ2scRGB, S_scRGB2sRGB16 }, -1 },
	{ LABS, GREY16, 4, { S_LabS2Lab, S_Lab2XYZ, S_XYZ2scRGB, S_scRGB2BW16 }, -1 },

	{ scRGB, XYZ, 1, { S_scRGB2XYZ }, -1 },
	{ scRGB, LAB, 2, { S_scRGB2XYZ, S_XYZ2Lab }, -1 },
	{ scRGB, LABS, 3, { S_scRGB2XYZ, S_XYZ2Lab, S_Lab2LabS }, -1 },
	{ scRGB, scRGB, 0, {}, VIPS_HIP_FORMAT_FLOAT },
	{ scRGB, sRGB, 1, { S_scRGB2sRGB }, -1 },
	{ scRGB, BW, 1, { S_scRGB2BW }, -1 },
	{ scRGB, RGB16, 1, { S_scRGB2sRGB16 }, -1 },
	{ scRGB, GREY16, 1, { S_scRGB2BW16 }, -1 },

	{ sRGB, XYZ, 2, { S_sRGB2scRGB, S_scRGB2XYZ }, -1 },
	{ sRGB, LAB, 3, { S_sRGB2scRGB, S_scRGB2XYZ, S_XYZ2Lab }, -1 },
	{ sRGB, LABS, 4, { S_sRGB2scRGB, S_scRGB2XYZ, S_XYZ2Lab, S_Lab2LabS }, -1 },
	{ sRGB, scRGB, 1, { S_sRGB2scRGB }, -1 },
	{ sRGB, sRGB, 0, {}, VIPS_HIP_FORMAT_UCHAR },
	{ sRGB, BW, 2, { S_sRGB2scRGB, S_scRGB2BW }, -1 },
	{ sRGB, RGB16, 1, { S_sRGB2RGB16 }, -1 },
	{ sRGB, GREY16, 2, { S_sRGB2scRGB, S_scRGB2BW16 }, -1 },

	// (B_W / GREY16 to XYZ, LAB, LABS, colourspace.c:395-400, 429-434: left out -- "no known route" for them is
	// pinned by tests/test_conv_colour_gpu.py::test_error_behaviour and by vips_sharpen of a two-band image)
	{ BW, scRGB, 2, { S_BW2sRGB, S_sRGB2scRGB }, -1 },
	{ BW, sRGB, 1, { S_BW2sRGB }, -1 },
	{ BW, BW, 0, {}, VIPS_HIP_FORMAT_UCHAR },
	{ BW, RGB16, 2, { S_BW2sRGB, S_sRGB2RGB16 }, -1 },
	{ BW, GREY16, 3, { S_BW2sRGB, S_sRGB2scRGB, S_scRGB2BW16 }, -1 },

	{ RGB16, XYZ, 2, { S_sRGB2scRGB, S_scRGB2XYZ }, -1 },
	{ RGB16, LAB, 3, { S_sRGB2scRGB, S_scRGB2XYZ, S_XYZ2Lab }, -1 },
	{ RGB16, LABS, 4, { S_sRGB2scRGB, S_scRGB2XYZ, S_XYZ2Lab, S_Lab2LabS }, -1 },
	{ RGB16, scRGB, 1, { S_sRGB2scRGB }, -1 },
	{ RGB16, sRGB, 1, { S_RGB162sRGB }, -1 },
	{ RGB16, BW, 2, { S_sRGB2scRGB, S_scRGB2BW }, -1 },
	{ RGB16, RGB16, 0, {}, VIPS_HIP_FORMAT_USHORT },
	{ RGB16, GREY16, 2, { S_sRGB2scRGB, S_scRGB2BW16 }, -1 },

	{ GREY16, scRGB, 2, { S_GREY162RGB16, S_sRGB2scRGB }, -1 },
	{ GREY16, sRGB, 2, { S_GREY162RGB16, S_RGB162sRGB }, -1 },
	{ GREY16, BW, 3, { S_GREY162RGB16, S_sRGB2scRGB, S_scRGB2BW }, -1 },
	{ GREY16, RGB16, 1, { S_GREY162RGB16 }, -1 },
	{ GREY16, GREY16, 0, {}, VIPS_HIP_FORMAT_USHORT },
};

#undef XYZ
#undef LAB
#undef LABS
#undef scRGB
#undef sRGB
#undef BW
#undef RGB16
#undef GREY16

inline bool step_replicates(int step)
{
	return step == VIPS_HIP_COLOUR_BW2sRGB || step == VIPS_HIP_COLOUR_GREY162RGB16;
}

inline bool step_shifts(int step)
{
	return step == VIPS_HIP_COLOUR_sRGB2RGB16 || step == VIPS_HIP_COLOUR_RGB162sRGB;
}

inline bool step_to_grey(int step)
{
	return step == VIPS_HIP_COLOUR_scRGB2BW || step == VIPS_HIP_COLOUR_scRGB2BW16;
}

} // namespace

const Route *vh::route_find(int from, int to)
{
	for (const Route &r : routes)
		if (r.from == from && r.to == to)
			return &r;
	return nullptr;
}

bool vh::route_is_plain(const Route &r)
{
	if (r.from == VIPS_HIP_INTERPRETATION_B_W || r.from == VIPS_HIP_INTERPRETATION_GREY16 ||
		r.from == VIPS_HIP_INTERPRETATION_RGB16)
		return false;
	for (int s = 0; s < r.n; s++)
		if (step_to_grey(r.steps[s]) || step_shifts(r.steps[s]))
			return false;
	return true;
}

int vh::step_out_interpretation(int step)
{
	switch (step) {
	case VIPS_HIP_COLOUR_sRGB2scRGB:
	case VIPS_HIP_COLOUR_sRGB2scRGB16:
	case VIPS_HIP_COLOUR_XYZ2scRGB:
		return VIPS_HIP_INTERPRETATION_scRGB;
	case VIPS_HIP_COLOUR_scRGB2XYZ:
	case VIPS_HIP_COLOUR_Lab2XYZ:
		return VIPS_HIP_INTERPRETATION_XYZ;
	case VIPS_HIP_COLOUR_XYZ2Lab:
	case VIPS_HIP_COLOUR_LabS2Lab:
		return VIPS_HIP_INTERPRETATION_LAB;
	case VIPS_HIP_COLOUR_scRGB2sRGB:
	case VIPS_HIP_COLOUR_BW2sRGB:
	case VIPS_HIP_COLOUR_RGB162sRGB:
		return VIPS_HIP_INTERPRETATION_sRGB;
	case VIPS_HIP_COLOUR_scRGB2sRGB16:
	case VIPS_HIP_COLOUR_GREY162RGB16:
	case VIPS_HIP_COLOUR_sRGB2RGB16:
		return VIPS_HIP_INTERPRETATION_RGB16;
	case VIPS_HIP_COLOUR_scRGB2BW:
		return VIPS_HIP_INTERPRETATION_B_W;
	case VIPS_HIP_COLOUR_scRGB2BW16:
		return VIPS_HIP_INTERPRETATION_GREY16;
	case VIPS_HIP_COLOUR_Lab2LabS:
		return VIPS_HIP_INTERPRETATION_LABS;
	default:
		return VIPS_HIP_INTERPRETATION_MULTIBAND;
	}
}

int vh::step_out_format(int step, int in_format)
{
	switch (step) {
	case VIPS_HIP_COLOUR_scRGB2sRGB:
	case VIPS_HIP_COLOUR_scRGB2BW:
	case VIPS_HIP_COLOUR_RGB162sRGB:
		return VIPS_HIP_FORMAT_UCHAR;
	case VIPS_HIP_COLOUR_scRGB2sRGB16:
	case VIPS_HIP_COLOUR_scRGB2BW16:
	case VIPS_HIP_COLOUR_sRGB2RGB16:
		return VIPS_HIP_FORMAT_USHORT;
	case VIPS_HIP_COLOUR_BW2sRGB:
	case VIPS_HIP_COLOUR_GREY162RGB16:
		return in_format;
	case VIPS_HIP_COLOUR_Lab2LabS: return VIPS_HIP_FORMAT_SHORT;
	default: return VIPS_HIP_FORMAT_FLOAT;
	}
}

int vh::cast_image(VipsHipImage *in, VipsHipImage **out, int format)
{
	// same format: vips_cast / vips_colourspace return the input (a pointer copy in the
	// reference).  Library-owned pixels are shared; caller-owned device memory is copied.
	if (format == in->format) {
		if (VipsHipImage *shared = image_share(in)) {
			*out = shared;
			return 0;
		}
		ImageRef c(vips_hip_image_new(in->width, in->height, in->bands, format, in->interpretation));
		if (!c.im || vips_hip_memcpy_d2d(c.im->data, in->data, in->stride * in->height))
			return -1;
		*out = c.release();
		return 0;
	}
	ImageRef o(vips_hip_image_new(in->width, in->height, in->bands, format, in->interpretation));
	if (!o.im)
		return -1;
	VipsHipRegion ri, ro;
	vips_hip_image_region(in, &ri);
	vips_hip_image_region(o.im, &ro);
	if (vips_hip_cast_gen(&ri, &ro))
		return -1;
	*out = o.release();
	return 0;
}

extern "C" {

int vips_hip_cast(VipsHipImage *in, VipsHipImage **out, int format)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error("cast", "null argument");
		return -1;
	}
	return cast_image(in, out, format);
}

static int premultiply_image(VipsHipImage *in, VipsHipImage **out, int uchar, int inverse)
{
	if (!in || !out) {
		error("premultiply", "null argument");
		return -1;
	}
	const char *domain = inverse ? "unpremultiply" : "premultiply";
	if (in->bands == 1) { // "Trivial case: fall back to copy()."
		return cast_image(in, out, in->format);
	}
	if (in->format == VIPS_HIP_FORMAT_DOUBLE) {
		error(domain, "double images are outside the HIP path");
		return -1;
	}
	const bool fast = uchar && in->format == VIPS_HIP_FORMAT_UCHAR;
	ImageRef o(vips_hip_image_new(in->width, in->height, in->bands,
		fast ? VIPS_HIP_FORMAT_UCHAR : VIPS_HIP_FORMAT_FLOAT, in->interpretation));
	if (!o.im)
		return -1;
	VipsHipRegion ri, ro;
	vips_hip_image_region(in, &ri);
	vips_hip_image_region(o.im, &ro);
	if (vips_hip_premultiply_gen(&ri, &ro, interpretation_max_alpha(in->interpretation), uchar, inverse))
		return -1;
	*out = o.release();
	return 0;
}

int vips_hip_premultiply(VipsHipImage *in, VipsHipImage **out, int uchar)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	return premultiply_image(in, out, uchar, 0);
}

int vips_hip_unpremultiply(VipsHipImage *in, VipsHipImage **out, int uchar)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	return premultiply_image(in, out, uchar, 1);
}

// vips_colourspace_build, colour/colourspace.c:551-612
int vips_hip_colourspace(VipsHipImage *in, VipsHipImage **out, int space)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error("colourspace", "null argument");
		return -1;
	}
	int interpretation = image_guess_interpretation(in);
	const Route *route = route_find(interpretation, space);
	if (!route) {
		error("vips_colourspace", "no known route from '%s' to '%s'",
			interpretation_nick(interpretation), interpretation_nick(space));
		return -1;
	}
	if (route->n == 0) {
		// vips_cast_float / vips_cast_uchar / vips_cast_short; interpretation unchanged
		return cast_image(in, out, route->cast_format);
	}
	// the route as it runs on THIS image: vips_sRGB2scRGB decodes at 16 bits when the image that enters it is
	// tagged RGB16 (sRGB2scRGB.c:115-123; GREY162RGB16 sets that tag), whatever its format
	int steps[5];
	const bool tag_decides = interpretation == VIPS_HIP_INTERPRETATION_B_W ||
		interpretation == VIPS_HIP_INTERPRETATION_GREY16 || interpretation == VIPS_HIP_INTERPRETATION_RGB16;
	{
		int tag = in->interpretation;
		for (int s = 0; s < route->n; s++) {
			steps[s] = route->steps[s];
			if (steps[s] == VIPS_HIP_COLOUR_sRGB2scRGB && tag_decides && tag == VIPS_HIP_INTERPRETATION_RGB16)
				steps[s] = VIPS_HIP_COLOUR_sRGB2scRGB16;
			tag = step_out_interpretation(steps[s]);
		}
	}
	const int first = steps[0];
	const int last = steps[route->n - 1];
	const int in_colour = step_replicates(first) ? 1 : 3;
	if (in->bands < in_colour) {
		error("colourspace", "image must have at least 3 bands");
		return -1;
	}
	bool any_shift = false;
	for (int s = 0; s < route->n; s++)
		any_shift |= step_shifts(steps[s]);
	if (any_shift && in->format != VIPS_HIP_FORMAT_UCHAR && in->format != VIPS_HIP_FORMAT_USHORT) {
		error("colourspace", "shift casts of band format %d are outside the HIP path", in->format);
		return -1;
	}

	// The stored input: the fused route kernel reads uchar / ushort / short / float and
	// applies the cast the first step's build() would insert; other formats get that
	// vips_cast as a pass of its own first.
	ImageRef pre;
	VipsHipImage *cur = in;
	const bool readable = cur->format == VIPS_HIP_FORMAT_UCHAR || cur->format == VIPS_HIP_FORMAT_USHORT ||
		cur->format == VIPS_HIP_FORMAT_SHORT || cur->format == VIPS_HIP_FORMAT_FLOAT;
	// (behind a band-replicating step the next step's cast: casting one band or its three copies is the same)
	const int decode = step_replicates(first) ? (route->n > 1 ? steps[1] : -1) : first;
	// The cast in front of a decoder narrows, and the reference casts the whole image, extra bands too, before it
	// splits them off (a float sRGB image's alpha of 159.2 leaves vips_sRGB2scRGB as 159): the kernel applies the
	// cast to the colour bands only, so an image with extra bands in another format than the decoder's is cast first.
	const int narrow = decode == VIPS_HIP_COLOUR_sRGB2scRGB ? VIPS_HIP_FORMAT_UCHAR
		: decode == VIPS_HIP_COLOUR_sRGB2scRGB16 ? VIPS_HIP_FORMAT_USHORT
		: decode == VIPS_HIP_COLOUR_LabS2Lab ? VIPS_HIP_FORMAT_SHORT : -1;
	if (!readable || (cur->bands > in_colour && narrow >= 0 && cur->format != narrow)) {
		if (decode < 0) {
			error("colourspace", "band format %d is outside the HIP path of this route", cur->format);
			return -1;
		}
		int want = VIPS_HIP_FORMAT_FLOAT;
		if (decode == VIPS_HIP_COLOUR_sRGB2scRGB)
			want = VIPS_HIP_FORMAT_UCHAR;
		else if (decode == VIPS_HIP_COLOUR_sRGB2scRGB16)
			want = VIPS_HIP_FORMAT_USHORT;
		else if (decode == VIPS_HIP_COLOUR_LabS2Lab)
			want = VIPS_HIP_FORMAT_SHORT;
		if (cast_image(cur, &pre.im, want))
			return -1;
		cur = pre.im;
	}

	// Grey to grey on a one-band image in its space's own format: the route is a function of one value, a table
	// (colour.hip grey_lut_image)
	if (cur->bands == 1 && step_replicates(first) && step_to_grey(last) &&
		cur->format == (first == VIPS_HIP_COLOUR_BW2sRGB ? VIPS_HIP_FORMAT_UCHAR : VIPS_HIP_FORMAT_USHORT)) {
		ImageRef o(vips_hip_image_new(cur->width, cur->height, 1, step_out_format(last), step_out_interpretation(last)));
		if (!o.im)
			return -1;
		VipsHipRegion ri, ro;
		vips_hip_image_region(cur, &ri);
		vips_hip_image_region(o.im, &ro);
		if (vh::grey_lut_image(&ri, &ro, first == VIPS_HIP_COLOUR_BW2sRGB))
			return -1;
		*out = o.release();
		return 0;
	}

	// Extra bands: every step rescales them in float when the alpha range changes
	// (vips_linear1) and casts them to its output format (colour.c:249-296).  Those
	// roundings do not compose, so images with extra bands run the chain one step per
	// pass like the reference; images with colour bands only take the fused route.
	const double alpha_scale = 1.0;
	const int extra = cur->bands - in_colour;
	const bool stepwise = extra > 0;

	if (!stepwise) {
		const int out_bands = step_to_grey(last) ? 1 : (any_shift && route->n == 1) ? cur->bands : 3;
		ImageRef o(vips_hip_image_new(cur->width, cur->height, out_bands, step_out_format(last, cur->format),
			step_out_interpretation(last)));
		if (!o.im)
			return -1;
		VipsHipRegion ri, ro;
		vips_hip_image_region(cur, &ri);
		vips_hip_image_region(o.im, &ro);
		if (vips_hip_colour_route_gen(steps, route->n, alpha_scale, &ri, &ro))
			return -1;
		*out = o.release();
		return 0;
	}

	// images with extra bands: one pass per step, exactly the reference's chain (the band-replicating steps copy
	// them, colourspace.c:115-150; the shift casts treat every band alike, :83-109)
	ImageRef hold;
	int before = interpretation;
	int colour = in_colour;
	for (int s = 0; s < route->n; s++) {
		const int st = steps[s];
		const int after = step_out_interpretation(st);
		if (step_replicates(st))
			colour = 3;
		else if (step_to_grey(st))
			colour = 1;
		ImageRef o(vips_hip_image_new(cur->width, cur->height, colour + extra, step_out_format(st, cur->format), after));
		if (!o.im)
			return -1;
		VipsHipRegion ri, ro;
		vips_hip_image_region(cur, &ri);
		vips_hip_image_region(o.im, &ro);
		const double scale = step_replicates(st) || step_shifts(st) ? 1.0 : interpretation_max_alpha(after) / interpretation_max_alpha(before);
		if (vips_hip_colour_route_gen(&st, 1, scale, &ri, &ro))
			return -1;
		vips_hip_image_unref(hold.im);
		hold.im = o.release();
		cur = hold.im;
		before = after;
	}
	*out = hold.release();
	return 0;
}

} // extern "C"
