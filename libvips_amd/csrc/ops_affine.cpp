// vips_affine, vips_similarity and vips_rotate (resample/affine.c, transform.c, similarity.c) on images in HBM: the host
// side -- vips_affine_build restated as a plan (inverse, default oarea, identity shortcut, range check, ink), the input
// rect a generate needs, the region checks, the premultiply chain, the C ABI.  The kernel is affine.hip.
#include "internal.h"

#include <climits>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <mutex>

using namespace vh;

struct _VipsHipAffinePlan {
	VipsHipAffine args;
	int width, height, bands, format, interpretation; // the input image
	double ia, ib, ic, id;
	int oarea[4];
	bool identity;
	bool chain;   // premultiply -> affine -> unpremultiply -> cast (affine.c:546-563, :614-619)
	int kformat;  // the format of the image the kernel resamples
	int window_size, window_offset;
	unsigned char ink[VIPS_HIP_AFFINE_MAX_PEL];
	unsigned char fill[VIPS_HIP_AFFINE_MAX_PEL]; // in `format`; premultiplied on first use when `chain`
	std::mutex mutex;
	bool fill_ready;
};

namespace {

struct PlanRef {
	VipsHipAffinePlan *p;
	~PlanRef() { vips_hip_affine_plan_free(p); }
};

void vector_to_ink(const double *background, int n_background, int bands, int format, unsigned char *dst)
{
	const int es = format_sizeof(format);
	for (int z = 0; z < bands; z++)
		element_to_format(background[n_background == bands ? z : 0], format, dst + (size_t) z * es);
}

struct Rect {
	int left, top, width, height;
};

// transform_rect, transform.c:186-222: the bounding box of the four mapped corners, rounded to nearest
template <typename F>
Rect transform_rect(const Rect &in, F point)
{
	double x1, y1, x2, y2, x3, y3, x4, y4;
	point((double) in.left, (double) in.top, &x1, &y1);
	point((double) in.left, (double) (in.top + in.height), &x3, &y3);
	point((double) (in.left + in.width), (double) in.top, &x2, &y2);
	point((double) (in.left + in.width), (double) (in.top + in.height), &x4, &y4);
	const double left = fmin(x1, fmin(x2, fmin(x3, x4)));
	const double right = fmax(x1, fmax(x2, fmax(x3, x4)));
	const double top = fmin(y1, fmin(y2, fmin(y3, y4)));
	const double bottom = fmax(y1, fmax(y2, fmax(y3, y4)));
	auto round_int = [](double r) { return (int) (r > 0 ? r + 0.5 : r - 0.5); };
	return Rect{round_int(left), round_int(top), round_int(right - left), round_int(bottom - top)};
}

// affine.c:264-303: the rect of the EMBEDDED input image the output rect reads, clipped to it
Rect need_embedded(const VipsHipAffinePlan *p, int left, int top, int width, int height)
{
	const Rect want{left + p->oarea[0], top + p->oarea[1], width, height};
	const double odx = p->args.odx, ody = p->args.ody;
	const double tidx = p->args.idx - 1, tidy = p->args.idy - 1; // affine.c:543-544
	Rect need = transform_rect(want, [&](double x, double y, double *ox, double *oy) {
		// vips__transform_invert_point, transform.c:171-181
		x -= odx;
		y -= ody;
		*ox = p->ia * x + p->ib * y - tidx;
		*oy = p->ic * x + p->id * y - tidy;
	});
	// the margin of 1, then the stencil
	need.left -= 1;
	need.top -= 1;
	need.width += 2 + p->window_size - 1;
	need.height += 2 + p->window_size - 1;
	const long long ew = (long long) p->width + p->window_size - 1 + 2, eh = (long long) p->height + p->window_size - 1 + 2;
	const long long x0 = need.left > 0 ? need.left : 0, y0 = need.top > 0 ? need.top : 0;
	long long x1 = (long long) need.left + need.width, y1 = (long long) need.top + need.height;
	x1 = x1 < ew ? x1 : ew;
	y1 = y1 < eh ? y1 : eh;
	if (x1 <= x0 || y1 <= y0)
		return Rect{0, 0, 0, 0};
	return Rect{(int) x0, (int) y0, (int) (x1 - x0), (int) (y1 - y0)};
}

} // namespace

namespace vh {

// one axis of the embedded rect [e0, e1] as pels of the image: what the fetch of affine.hip and mapim.hip reads for it
void embedded_axis_to_image(int extend, int off, int size, int e0, int e1, int *p0, int *p1)
{
	const bool border = e0 < off || e1 >= off + size;
	if (border && (extend == VIPS_HIP_EXTEND_REPEAT || extend == VIPS_HIP_EXTEND_MIRROR)) {
		*p0 = 0;
		*p1 = size - 1;
		return;
	}
	const int a = e0 - off, b = e1 - off;
	*p0 = a < 0 ? 0 : (a > size - 1 ? size - 1 : a);
	*p1 = b < 0 ? 0 : (b > size - 1 ? size - 1 : b);
}

int resample_check(const char *domain, int interpolate, int extend, int format)
{
	if (interpolate < VIPS_HIP_INTERPOLATE_NEAREST || interpolate > VIPS_HIP_INTERPOLATE_BICUBIC) {
		error(domain, "interpolator %d is outside the HIP path (nearest, bilinear, bicubic)", interpolate);
		return -1;
	}
	if (extend < VIPS_HIP_EXTEND_BLACK || extend > VIPS_HIP_EXTEND_BACKGROUND) {
		error(domain, "enum 'VipsExtend' has no member %d", extend);
		return -1;
	}
	if (format_iscomplex(format)) {
		error(domain, "complex images are outside the HIP path");
		return -1;
	}
	if (format == VIPS_HIP_FORMAT_DOUBLE) {
		error(domain, "double images are outside the HIP path");
		return -1;
	}
	if (format_sizeof(format) == 0) {
		error(domain, "unknown band format %d", format);
		return -1;
	}
	return 0;
}

int resample_pels(const char *domain, int interpolate, int extend, int premultiplied, int n_background, const double *background,
	int bands, int format, int interpretation, ResamplePels *p)
{
	p->window_size = interpolate == VIPS_HIP_INTERPOLATE_NEAREST ? 1 : interpolate == VIPS_HIP_INTERPOLATE_BILINEAR ? 2 : 4;
	p->window_offset = p->window_size / 2 - 1 > 0 ? p->window_size / 2 - 1 : 0; // interpolate.c:150-167
	p->chain = false;
	p->kformat = format;
	p->fill_ready = true;
	memset(p->ink, 0, sizeof(p->ink));
	memset(p->fill, 0, sizeof(p->fill));
	// vips__vector_to_ink -> vips_linear -> vips_check_vector, iofuncs/error.c:1118-1140
	if (n_background < 1 || n_background > VIPS_HIP_AFFINE_MAX_BACKGROUND || !(n_background == bands || n_background == 1 || bands == 1)) {
		if (bands == 1)
			error("linear", "vector must have 1 element");
		else
			error("linear", "vector must have 1 or %d elements", bands);
		return -1;
	}
	const int ibands = interpretation_bands(interpretation);
	p->chain = ibands > 0 && bands > ibands && !premultiplied;
	if (p->chain)
		p->kformat = VIPS_HIP_FORMAT_FLOAT;
	if ((long long) bands * format_sizeof(p->kformat) > VIPS_HIP_AFFINE_MAX_PEL) {
		error(domain, "pels of more than %d bytes are outside the HIP path", VIPS_HIP_AFFINE_MAX_PEL);
		return -1;
	}
	// the pel the embed paints round the image (embed.c:270-298), in the image's own format
	const size_t pel = (size_t) bands * format_sizeof(format);
	if (extend == VIPS_HIP_EXTEND_WHITE) {
		// vips_region_paint (iofuncs/region.c:909-956): memset for the integer formats, the value for float
		const int white = (int) interpretation_max_alpha(interpretation);
		if (format == VIPS_HIP_FORMAT_FLOAT) {
			const float v = (float) white;
			for (int z = 0; z < bands; z++)
				memcpy(p->fill + (size_t) z * sizeof(float), &v, sizeof(float));
		}
		else
			memset(p->fill, white, pel);
	}
	else if (extend == VIPS_HIP_EXTEND_BACKGROUND)
		vector_to_ink(background, n_background, bands, format, p->fill);
	p->fill_ready = !p->chain;
	// the ink of what the clip rejects, in the format of the resampled image and not premultiplied (affine.c:565-571)
	vector_to_ink(background, n_background, bands, p->kformat, p->ink);
	return 0;
}

// the fill pel of the premultiplied image: the image's own pel through vips_premultiply (the embed comes first,
// affine.c:530-563, mapim.c:472-498)
int resample_fill_premultiply(const char *domain, ResamplePels *p, int bands, int format, int interpretation)
{
	if (p->fill_ready)
		return 0;
	ImageRef one(vips_hip_image_new_from_memory(p->fill, 1, 1, bands, format, interpretation));
	ImageRef pre;
	if (!one.im || vips_hip_premultiply(one.im, &pre.im, 0))
		return -1;
	if (pre.im->format != VIPS_HIP_FORMAT_FLOAT) {
		error(domain, "premultiply did not make a float image");
		return -1;
	}
	memset(p->fill, 0, sizeof(p->fill));
	if (vips_hip_image_write_to_memory(pre.im, p->fill))
		return -1;
	p->fill_ready = true;
	return 0;
}

} // namespace vh

extern "C" {

void vips_hip_affine_defaults(VipsHipAffine *args)
{
	if (!args)
		return;
	memset(args, 0, sizeof(*args));
	args->a = 1.0;
	args->d = 1.0;
	args->interpolate = VIPS_HIP_INTERPOLATE_BILINEAR;
	args->extend = VIPS_HIP_EXTEND_BACKGROUND;
	args->n_background = 1;
}

VipsHipAffinePlan *vips_hip_affine_plan_new(const VipsHipAffine *args, int width, int height, int bands, int format,
	int interpretation)
{
	const char *domain = "affine";
	if (!args || width < 1 || height < 1 || bands < 1) {
		error(domain, "bad arguments");
		return nullptr;
	}
	if (resample_check(domain, args->interpolate, args->extend, format))
		return nullptr;
	// vips__transform_calc_inverse, transform.c:52-72
	const double det = args->a * args->d - args->b * args->c;
	if (fabs(det) < 2.0 * DBL_MIN) {
		error("vips__transform_calc_inverse", "singular or near-singular matrix");
		return nullptr;
	}
	std::unique_ptr<VipsHipAffinePlan> p(new VipsHipAffinePlan);
	p->args = *args;
	p->width = width;
	p->height = height;
	p->bands = bands;
	p->format = format;
	p->interpretation = interpretation;
	const double tmp = 1.0 / det;
	p->ia = tmp * args->d;
	p->ib = -tmp * args->b;
	p->ic = -tmp * args->c;
	p->id = tmp * args->a;
	// vips__transform_set_area (transform.c:248-252) with every displacement still 0, then the caller's oarea
	const Rect area = transform_rect(Rect{0, 0, width, height}, [&](double x, double y, double *ox, double *oy) {
		x += 0.0;
		y += 0.0;
		*ox = args->a * x + args->b * y + 0.0;
		*oy = args->c * x + args->d * y + 0.0;
	});
	p->oarea[0] = area.left;
	p->oarea[1] = area.top;
	p->oarea[2] = area.width;
	p->oarea[3] = area.height;
	if (args->have_oarea)
		memcpy(p->oarea, args->oarea, sizeof(p->oarea));
	// affine.c:499-504
	p->identity = args->a == 1.0 && args->b == 0.0 && args->c == 0.0 && args->d == 1.0 && args->idx == 0.0 && args->idy == 0.0 &&
		args->odx == 0.0 && args->ody == 0.0 && p->oarea[0] == 0 && p->oarea[1] == 0 && p->oarea[2] == width && p->oarea[3] == height;
	p->window_size = args->interpolate == VIPS_HIP_INTERPOLATE_NEAREST ? 1 : args->interpolate == VIPS_HIP_INTERPOLATE_BILINEAR ? 2 : 4;
	p->window_offset = p->window_size / 2 - 1 > 0 ? p->window_size / 2 - 1 : 0; // interpolate.c:150-167
	p->chain = false;
	p->kformat = format;
	p->fill_ready = true;
	memset(p->ink, 0, sizeof(p->ink));
	memset(p->fill, 0, sizeof(p->fill));
	if (p->identity)
		return p.release();
	// affine.c:507-518
	const int edge = INT_MAX / 64;
	if (p->oarea[0] < -edge || p->oarea[1] < -edge ||
		(unsigned long long) (long long) p->oarea[0] + (unsigned long long) (long long) p->oarea[2] > (unsigned long long) edge ||
		(unsigned long long) (long long) p->oarea[1] + (unsigned long long) (long long) p->oarea[3] > (unsigned long long) edge) {
		error(domain, "output coordinates out of range");
		return nullptr;
	}
	if (p->oarea[2] < 1 || p->oarea[3] < 1) {
		error("VipsImage", "bad dimensions");
		return nullptr;
	}
	// the ink, the embed's fill pel and the premultiply chain
	ResamplePels pels;
	if (resample_pels(domain, args->interpolate, args->extend, args->premultiplied, args->n_background, args->background, bands, format,
			interpretation, &pels))
		return nullptr;
	p->chain = pels.chain;
	p->kformat = pels.kformat;
	p->fill_ready = pels.fill_ready;
	memcpy(p->ink, pels.ink, sizeof(p->ink));
	memcpy(p->fill, pels.fill, sizeof(p->fill));
	return p.release();
}

void vips_hip_affine_plan_free(VipsHipAffinePlan *plan)
{
	delete plan;
}

int vips_hip_affine_plan_get(const VipsHipAffinePlan *plan, int what)
{
	if (!plan)
		return -1;
	switch (what) {
	case 0: return plan->identity ? plan->width : plan->oarea[2];
	case 1: return plan->identity ? plan->height : plan->oarea[3];
	case 2: return plan->identity ? 1 : 0;
	case 3:
		// affine.c:573-580: FATSTRIP for a pure scale, else SMALLTILE -- and a pipeline takes the smallest hint of its
		// inputs (iofuncs/image.c, vips__demand_hint_array): the embed of extend repeat and mirror is built on
		// vips_replicate, which is SMALLTILE (conversion/replicate.c:166), so those are tiles whatever the matrix
		return !plan->args.force_tiles && plan->args.b == 0.0 && plan->args.c == 0.0 && plan->args.extend != VIPS_HIP_EXTEND_REPEAT &&
				plan->args.extend != VIPS_HIP_EXTEND_MIRROR
			? 0
			: 128;
	case 4: return plan->chain ? 1 : 0;
	case 5: return plan->kformat;
	default: return -1;
	}
}

void vips_hip_affine_need(const VipsHipAffinePlan *plan, int left, int top, int width, int height, int in[4])
{
	if (!in)
		return;
	in[0] = in[1] = in[2] = in[3] = 0;
	if (!plan || width < 1 || height < 1)
		return;
	const Rect e = need_embedded(plan, left, top, width, height);
	if (e.width < 1 || e.height < 1)
		return;
	const int off = plan->window_offset + 1;
	int x0, x1, y0, y1;
	embedded_axis_to_image(plan->args.extend, off, plan->width, e.left, e.left + e.width - 1, &x0, &x1);
	embedded_axis_to_image(plan->args.extend, off, plan->height, e.top, e.top + e.height - 1, &y0, &y1);
	in[0] = x0;
	in[1] = y0;
	in[2] = x1 - x0 + 1;
	in[3] = y1 - y0 + 1;
}

int vips_hip_affine_gen(VipsHipAffinePlan *plan, const VipsHipRegion *in, const VipsHipRegion *out, int tile_width)
{
	const char *domain = "affine";
	if (ensure_init())
		return -1;
	if (!plan || !in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (plan->identity) {
		error(domain, "the identity transform is a copy: there is nothing to generate");
		return -1;
	}
	if (in->format != plan->kformat || out->format != plan->kformat || in->bands != plan->bands || out->bands != plan->bands) {
		error(domain, "regions must have the plan's bands and format");
		return -1;
	}
	if (in->im_width != plan->width || in->im_height != plan->height || out->im_width != plan->oarea[2] ||
		out->im_height != plan->oarea[3]) {
		error(domain, "regions must belong to the plan's images");
		return -1;
	}
	if (in->left < 0 || in->top < 0 || (long long) in->left + in->width > in->im_width || (long long) in->top + in->height > in->im_height ||
		out->left < 0 || out->top < 0 || (long long) out->left + out->width > out->im_width ||
		(long long) out->top + out->height > out->im_height) {
		error(domain, "region outside its image");
		return -1;
	}
	if (tile_width < 0 || tile_width > 1024) {
		error(domain, "tile_width should be 0 .. 1024");
		return -1;
	}
	if (tile_width == 0 && !(plan->args.b == 0.0 && plan->args.c == 0.0)) {
		error(domain, "whole-row rects need b == c == 0");
		return -1;
	}
	int need[4];
	vips_hip_affine_need(plan, out->left, out->top, out->width, out->height, need);
	const bool all_ink = need[2] == 0 || need[3] == 0;
	if (!all_ink && (need[0] < in->left || need[1] < in->top || need[0] + need[2] > in->left + in->width ||
						need[1] + need[3] > in->top + in->height)) {
		error(domain, "input region too small");
		return -1;
	}
	// the fill pel of the premultiplied image: the image's own pel through vips_premultiply (the embed comes first,
	// affine.c:530-563), once
	{
		std::lock_guard<std::mutex> lock(plan->mutex);
		if (!plan->fill_ready) {
			ResamplePels pels;
			pels.fill_ready = false;
			memcpy(pels.fill, plan->fill, sizeof(pels.fill));
			if (resample_fill_premultiply(domain, &pels, plan->bands, plan->format, plan->interpretation))
				return -1;
			memcpy(plan->fill, pels.fill, sizeof(plan->fill));
			plan->fill_ready = true;
		}
	}
	AffineArgs a;
	memset(&a, 0, sizeof(a));
	a.in = (const unsigned char *) in->data;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) out->stride;
	a.in_left = in->left;
	a.in_top = in->top;
	a.in_width = all_ink ? 0 : in->width;
	a.in_height = all_ink ? 0 : in->height;
	a.im_width = plan->width;
	a.im_height = plan->height;
	a.out_left = out->left;
	a.out_top = out->top;
	a.out_width = out->width;
	a.out_height = out->height;
	a.bands = plan->bands;
	a.window_offset = plan->window_offset;
	a.extend = plan->args.extend;
	a.tile_width = tile_width;
	a.oarea_left = plan->oarea[0];
	a.oarea_top = plan->oarea[1];
	a.ia = plan->ia;
	a.ib = plan->ib;
	a.ic = plan->ic;
	a.id = plan->id;
	a.odx = plan->args.odx;
	a.ody = plan->args.ody;
	a.tidx = plan->args.idx - 1; // affine.c:543-544: the one-pel border of the embed
	a.tidy = plan->args.idy - 1;
	memcpy(a.ink, plan->ink, sizeof(a.ink));
	memcpy(a.fill, plan->fill, sizeof(a.fill));
	return affine_run(domain, a, plan->kformat, plan->args.interpolate);
}

// vips_affine_build, affine.c:412-625
int vips_hip_affine(VipsHipImage *in, VipsHipImage **out, const VipsHipAffine *args)
{
	const char *domain = "affine";
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out || !args) {
		error(domain, "null argument");
		return -1;
	}
	PlanRef plan{vips_hip_affine_plan_new(args, in->width, in->height, in->bands, in->format, in->interpretation)};
	if (!plan.p)
		return -1;
	if (plan.p->identity) // affine.c:499-504: vips_image_write, a pointer copy
		return vips_hip_cast(in, out, in->format);
	ImageRef pre;
	VipsHipImage *src = in;
	if (plan.p->chain) {
		if (vips_hip_premultiply(in, &pre.im, 0))
			return -1;
		src = pre.im;
	}
	ImageRef o(vips_hip_image_new(plan.p->oarea[2], plan.p->oarea[3], in->bands, plan.p->kformat, in->interpretation));
	if (!o.im)
		return -1;
	VipsHipRegion ri, ro;
	vips_hip_image_region(src, &ri);
	vips_hip_image_region(o.im, &ro);
	if (vips_hip_affine_gen(plan.p, &ri, &ro, vips_hip_affine_plan_get(plan.p, 3)))
		return -1;
	if (plan.p->chain) {
		ImageRef un, back;
		if (vips_hip_unpremultiply(o.im, &un.im, 0) || vips_hip_cast(un.im, &back.im, in->format))
			return -1;
		*out = back.release();
		return 0;
	}
	*out = o.release();
	return 0;
}

// vips_similarity_base_build, similarity.c:82-111
int vips_hip_similarity(VipsHipImage *in, VipsHipImage **out, double scale, double angle, const VipsHipAffine *args)
{
	VipsHipAffine a;
	if (args)
		a = *args;
	else
		vips_hip_affine_defaults(&a);
	const double rad = ((angle / 360.0) * 2.0 * 3.14159265358979323846); // VIPS_RAD
	a.a = scale * cos(rad);
	a.b = scale * -sin(rad);
	a.c = -a.b;
	a.d = a.a;
	return vips_hip_affine(in, out, &a);
}

int vips_hip_rotate(VipsHipImage *in, VipsHipImage **out, double angle, const VipsHipAffine *args)
{
	return vips_hip_similarity(in, out, 1.0, angle, args);
}

} // extern "C"
