// vips_sobel / vips_scharr / vips_prewitt (convolution/edge.c) and vips_compass (compass.c) on images in HBM: the host
// side -- the plans that restate vips_edge_build (the three fixed masks, rot90, which path runs and what it puts out)
// and vips_compass_build (vips_rot45 of the mask, the collapse of `times` onto the rotation's period, the output
// format), the region checks, the C ABI.  The kernels are edge.hip; the general tier's convolutions are conv.hip's and
// approx.hip's.
#include "internal.h"

#include <cmath>
#include <mutex>
#include <vector>

using namespace vh;

namespace {

struct ConvRef {
	VipsHipConv *c;
	explicit ConvRef(VipsHipConv *conv)
		: c(conv)
	{
	}
	~ConvRef() { vips_hip_conv_free(c); }
};

// vips_sobel_build, vips_scharr_build, vips_prewitt_build: edge.c:247-250, 280-283, 313-316
const double edge_masks[VIPS_HIP_EDGE_LAST][9] = {
	{ 1.0, 2.0, 1.0, 0.0, 0.0, 0.0, -1.0, -2.0, -1.0 },
	{ -3.0, 0.0, 3.0, -10.0, 0.0, 10.0, -3.0, 0.0, 3.0 },
	{ -1.0, 0.0, 1.0, -1.0, 0.0, 1.0, -1.0, 0.0, 1.0 },
};
const char *const edge_names[VIPS_HIP_EDGE_LAST] = { "sobel", "scharr", "prewitt" };

// vips_rot90 of a square matrix (conversion/rot.c): a quarter turn clockwise, out(x, y) = in(y, n - 1 - x)
void mask_rot90(const double *in, int n, double *out)
{
	for (int y = 0; y < n; y++)
		for (int x = 0; x < n; x++)
			out[y * n + x] = in[(n - 1 - x) * n + y];
}

// One vips_rot45_rot45 (conversion/rot45.c:104-180): the eight triangles of an odd square matrix each move on to the
// next, the centre stays.  Pure index movement; eight of them are the identity.
void mask_rot45(const double *in, int size, double *out)
{
	const int size_2 = size / 2;
	auto at = [size](int x, int y) { return y * size + x; };
	for (int y = 0; y < size_2; y++)
		for (int x = y; x < size_2; x++) {
			out[at(x, y)] = in[at(y, size_2 - (x - y))];                                      // 1 from 8
			out[at(y, size_2 - (x - y))] = in[at(y, (size - 1) - x)];                         // 8 from 7
			out[at(y, (size - 1) - x)] = in[at(size_2 - (x - y), (size - 1) - y)];            // 7 from 6
			out[at(size_2 - (x - y), (size - 1) - y)] = in[at((size - 1) - x, (size - 1) - y)]; // 6 from 5
			out[at((size - 1) - x, (size - 1) - y)] = in[at((size - 1) - y, (x - y) + size_2)]; // 5 from 4
			out[at((size - 1) - y, (x - y) + size_2)] = in[at((size - 1) - y, x)];            // 4 from 3
			out[at((size - 1) - y, x)] = in[at((x - y) + size_2, y)];                         // 3 from 2
			out[at((x - y) + size_2, y)] = in[at(x, y)];                                      // 2 from 1
		}
	out[at(size_2, size_2)] = in[at(size_2, size_2)];
}

int sum_format(int format)
{
	// vips_sum_format_table, arithmetic/sum.c:137-140
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR:
	case VIPS_HIP_FORMAT_USHORT:
	case VIPS_HIP_FORMAT_UINT:
		return VIPS_HIP_FORMAT_UINT;
	case VIPS_HIP_FORMAT_CHAR:
	case VIPS_HIP_FORMAT_SHORT:
	case VIPS_HIP_FORMAT_INT:
		return VIPS_HIP_FORMAT_INT;
	default:
		return format;
	}
}

} // namespace

// The counter of the float canny kernel, one a device: made on first use, never freed.
static std::mutex canny_mutex;
static unsigned int *canny_counters[64];

static unsigned int *canny_counter()
{
	const int device = current_device();
	if (device < 0 || device >= 64)
		return nullptr;
	std::lock_guard<std::mutex> lock(canny_mutex);
	if (!canny_counters[device]) {
		unsigned int *p = (unsigned int *) vips_hip_malloc(sizeof(unsigned int));
		if (!p)
			return nullptr;
		hipError_t err = hipMemsetAsync(p, 0, sizeof(unsigned int), stream());
		if (err == hipSuccess)
			err = hipStreamSynchronize(stream());
		if (err != hipSuccess) {
			hip_failed(err, "clearing the canny counter");
			vips_hip_free(p);
			return nullptr;
		}
		canny_counters[device] = p;
	}
	return canny_counters[device];
}

// vips_compass_build restated, compass.c:65-147
struct _VipsHipCompass {
	int size; // the mask's side
	int times, angle, combine, precision, layers, cluster;
	double scale, offset;
	int n;                                   // distinct masks: min(times, the period of the rotation)
	std::vector<std::vector<double>> masks;  // mask k = the mask turned k times by `angle`
	int mult[8];                             // how many of the `times` convolutions run mask k
};

extern "C" {

// vips_edge_build, edge.c:185-203: uchar takes the integer path, everything else the float one
int vips_hip_edge_gen(const VipsHipRegion *in, const VipsHipRegion *out, int edge)
{
	if (ensure_init())
		return -1;
	if (edge < 0 || edge >= VIPS_HIP_EDGE_LAST) {
		error("edge", "edge should be 0 (sobel), 1 (scharr) or 2 (prewitt)");
		return -1;
	}
	const char *domain = edge_names[edge];
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (format_iscomplex(in->format)) {
		error(domain, "complex images are outside the HIP path");
		return -1;
	}
	if (in->format == VIPS_HIP_FORMAT_DOUBLE) {
		error(domain, "double images are outside the HIP path");
		return -1;
	}
	if (out->format != VIPS_HIP_FORMAT_UCHAR) {
		error(domain, "the output is uchar");
		return -1;
	}
	const double *mask = edge_masks[edge];
	double mask90[9];
	mask_rot90(mask, 3, mask90);
	NbArgs a;
	if (nb_geometry(domain, in, out, 3, 3, &a))
		return -1;
	const bool uchar = in->format == VIPS_HIP_FORMAT_UCHAR;
	// the fused kernel is the arithmetic of convi's C path (not of its Highway variant, when that is selected)
	if (uchar && !vips_hip_vector_isenabled() && edge_u8_fits(in->bands)) {
		int m[9], m90[9];
		for (int i = 0; i < 9; i++) {
			m[i] = (int) rint(mask[i]); // vips__image_intize, convi.c:892-895
			m90[i] = (int) rint(mask90[i]);
		}
		return edge_u8_run(domain, a, m, m90);
	}
	// The general tier: each mask through the conv kernels as its own mask (uchar: precision integer, scale 2, offset
	// 128, edge.c:123-135; else the default precision, float, :165-167), then the combine.
	const int precision = uchar ? VIPS_HIP_PRECISION_INTEGER : VIPS_HIP_PRECISION_FLOAT;
	const double scale = uchar ? 2.0 : 1.0, offset = uchar ? 128.0 : 0.0;
	ConvRef c1(vips_hip_conv_new(mask, 3, 3, scale, offset, precision));
	ConvRef c2(vips_hip_conv_new(mask90, 3, 3, scale, offset, precision));
	if (!c1.c || !c2.c)
		return -1;
	VipsHipRegion t = *out;
	t.format = vips_hip_conv_out_format(c1.c, in->format);
	t.stride = (size_t) out->width * out->bands * format_sizeof(t.format);
	DeviceBlock b1(t.stride * out->height), b2(t.stride * out->height);
	if (!b1.p || !b2.p)
		return -1;
	t.data = b1.p;
	if (vips_hip_conv_gen(c1.c, in, &t))
		return -1;
	t.data = b2.p;
	if (vips_hip_conv_gen(c2.c, in, &t))
		return -1;
	// (the blocks and the plans' tables go back to the pool behind the kernels: the pool hands them out again on this
	// thread's stream only)
	return edge_combine_run(domain, b1.p, (long long) t.stride, b2.p, (long long) t.stride, out->data, (long long) out->stride,
		(long long) out->width * out->bands, out->height, !uchar);
}

void vips_hip_edge_need(int top, int height, int *in_top, int *in_height)
{
	if (in_top)
		*in_top = top - 1;
	if (in_height)
		*in_height = height + 2;
}

int vips_hip_edge_step(int what)
{
	return what == 6 ? edge_tile(3) : what < 3 ? edge_tile(what) : canny_tile(what - 3);
}

static int edge_image(VipsHipImage *in, VipsHipImage **out, int edge)
{
	const char *domain = edge_names[edge];
	if (enter(domain, in, out))
		return -1;
	// both paths end in uchar: vips_edge_uchar_gen writes the conv's format, the float path vips_cast_uchar (edge.c:174)
	return whole_image(in, out, in->bands, VIPS_HIP_FORMAT_UCHAR,
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_edge_gen(ri, ro, edge); });
}

int vips_hip_sobel(VipsHipImage *in, VipsHipImage **out)
{
	return edge_image(in, out, VIPS_HIP_EDGE_SOBEL);
}

int vips_hip_scharr(VipsHipImage *in, VipsHipImage **out)
{
	return edge_image(in, out, VIPS_HIP_EDGE_SCHARR);
}

int vips_hip_prewitt(VipsHipImage *in, VipsHipImage **out)
{
	return edge_image(in, out, VIPS_HIP_EDGE_PREWITT);
}

// vips_rot45 of a matrix (conversion/rot45.c:182-250): @angle 45-degree steps
int vips_hip_rot45(const double *in, int width, int height, int angle, double *out)
{
	if (!in || !out || width < 1 || height < 1) {
		error("rot45", "null argument");
		return -1;
	}
	if (width != height || width % 2 == 0) { // vips_check_oddsquare, iofuncs/error.c:956-967
		error("rot45", "images must be odd and square");
		return -1;
	}
	if (angle < VIPS_HIP_ANGLE45_D0 || angle > VIPS_HIP_ANGLE45_D315) {
		error("rot45", "angle should be 0 (d0) .. 7 (d315)");
		return -1;
	}
	std::vector<double> a(in, in + (size_t) width * width), b(a.size());
	for (int i = 0; i < angle; i++) {
		mask_rot45(a.data(), width, b.data());
		a.swap(b);
	}
	for (size_t i = 0; i < a.size(); i++)
		out[i] = a[i];
	return 0;
}

VipsHipCompass *vips_hip_compass_new(const double *mask, int mask_width, int mask_height, double scale, double offset,
	int times, int angle, int combine, int precision, int layers, int cluster)
{
	const char *domain = "compass";
	if (!mask || mask_width < 1 || mask_height < 1) {
		error(domain, "bad mask");
		return nullptr;
	}
	if (times < 1 || times > 1000) {
		error(domain, "times should be 1 .. 1000");
		return nullptr;
	}
	if (angle < VIPS_HIP_ANGLE45_D0 || angle > VIPS_HIP_ANGLE45_D315) {
		error(domain, "angle should be 0 (d0) .. 7 (d315)");
		return nullptr;
	}
	if (combine != VIPS_HIP_COMBINE_MAX && combine != VIPS_HIP_COMBINE_SUM && combine != VIPS_HIP_COMBINE_MIN) {
		error(domain, "combine should be 0 (max), 1 (sum) or 2 (min)");
		return nullptr;
	}
	if (precision != VIPS_HIP_PRECISION_INTEGER && precision != VIPS_HIP_PRECISION_FLOAT &&
		precision != VIPS_HIP_PRECISION_APPROXIMATE) {
		error(domain, "precision should be 0 (integer), 1 (float) or 2 (approximate)");
		return nullptr;
	}
	// every mask is turned once behind its convolution, the last one too (compass.c:93-106): the check of vips_rot45
	// meets every call
	if (mask_width != mask_height || mask_width % 2 == 0) {
		error("rot45", "images must be odd and square");
		return nullptr;
	}
	VipsHipCompass *p = new VipsHipCompass;
	p->size = mask_width;
	p->times = times;
	p->angle = angle;
	p->combine = combine;
	p->precision = precision;
	p->layers = layers;
	p->cluster = cluster;
	p->scale = scale;
	p->offset = offset;
	// `angle` steps of 45 degrees a turn, eight steps the identity: the sequence of masks has period 8 / gcd(8, angle)
	int period = 1;
	while ((period * angle) % 8 != 0)
		period++;
	p->n = times < period ? times : period;
	std::vector<double> m(mask, mask + (size_t) mask_width * mask_width);
	for (int k = 0; k < p->n; k++) {
		p->masks.push_back(m);
		std::vector<double> next(m.size());
		vips_hip_rot45(m.data(), mask_width, mask_width, angle, next.data());
		m.swap(next);
	}
	for (int k = 0; k < 8; k++)
		p->mult[k] = k < p->n ? (times - k + p->n - 1) / p->n : 0;
	return p;
}

void vips_hip_compass_free(VipsHipCompass *plan)
{
	delete plan;
}

int vips_hip_compass_get_masks(const VipsHipCompass *plan, double *masks, int *mult, int max)
{
	if (!plan) {
		error("compass", "null plan");
		return -1;
	}
	const int ne = plan->size * plan->size;
	for (int k = 0; k < plan->n && k < max; k++) {
		if (masks)
			for (int i = 0; i < ne; i++)
				masks[k * ne + i] = plan->masks[k][i];
		if (mult)
			mult[k] = plan->mult[k];
	}
	return plan->n;
}

// the convolution's format (conv.c:88-108: convi and conva keep it, convf makes float), kept by vips_abs and
// vips_bandrank, widened by vips_sum
int vips_hip_compass_out_format(const VipsHipCompass *plan, int format)
{
	if (!plan)
		return -1;
	int f = format;
	if (plan->precision == VIPS_HIP_PRECISION_FLOAT && f != VIPS_HIP_FORMAT_DOUBLE && !format_iscomplex(f))
		f = VIPS_HIP_FORMAT_FLOAT;
	return plan->combine == VIPS_HIP_COMBINE_SUM ? sum_format(f) : f;
}

// 1: the fused kernel runs these regions
static int compass_fused(const VipsHipCompass *plan, const VipsHipRegion *in, std::vector<int> *masks, int *scale, int *offset)
{
	if (in->format != VIPS_HIP_FORMAT_UCHAR || plan->precision != VIPS_HIP_PRECISION_INTEGER || plan->size != 3 ||
		vips_hip_vector_isenabled())
		return 0;
	// vips_convi_build: the elements rint()ed (convi.c:892-895), scale and offset the mask's own, rint()ed (:760-762)
	masks->clear();
	for (int k = 0; k < plan->n; k++)
		for (int i = 0; i < 9; i++) {
			const double v = rint(plan->masks[k][i]);
			if (!(v >= -100000 && v <= 100000))
				return 0;
			masks->push_back((int) v);
		}
	const double s = rint(plan->scale), o = rint(plan->offset);
	if (!(s >= -(1 << 28) && s <= (1 << 28)) || !(o >= -(1 << 28) && o <= (1 << 28)))
		return 0;
	*scale = (int) s;
	*offset = (int) o;
	return compass_u8_takes(in->bands, masks->data(), plan->n, *scale);
}

int vips_hip_compass_gen(const VipsHipCompass *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = "compass";
	if (ensure_init())
		return -1;
	if (!plan) {
		error(domain, "null plan");
		return -1;
	}
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (format_iscomplex(in->format)) {
		error(domain, "complex images are outside the HIP path");
		return -1;
	}
	if (in->format == VIPS_HIP_FORMAT_DOUBLE) {
		error(domain, "double images are outside the HIP path");
		return -1;
	}
	if (out->format != vips_hip_compass_out_format(plan, in->format)) {
		error(domain, "output region has the wrong format");
		return -1;
	}
	NbArgs a;
	if (nb_geometry(domain, in, out, plan->size, plan->size, &a))
		return -1;
	std::vector<int> imasks;
	int scale_i = 1, offset_i = 0;
	if (compass_fused(plan, in, &imasks, &scale_i, &offset_i))
		return compass_u8_run(domain, a, imasks.data(), plan->mult, plan->n, scale_i, offset_i, plan->combine);
	// The general tier: every distinct mask through the convolution of its precision as its own mask (rot45 carries
	// scale and offset along), each into a plane of its own, then abs and the combine.
	VipsHipRegion t = *out;
	t.format = plan->precision == VIPS_HIP_PRECISION_FLOAT ? VIPS_HIP_FORMAT_FLOAT : in->format;
	t.stride = ((size_t) out->width * out->bands * format_sizeof(t.format) + 15) / 16 * 16;
	const size_t plane = t.stride * out->height;
	DeviceBlock block(plane * plan->n);
	if (!block.p)
		return -1;
	for (int k = 0; k < plan->n; k++) {
		t.data = (char *) block.p + plane * k;
		if (plan->precision == VIPS_HIP_PRECISION_APPROXIMATE) {
			VipsHipConva *c = vips_hip_conva_new(plan->masks[k].data(), plan->size, plan->size, plan->scale, plan->offset,
				plan->layers, plan->cluster);
			if (!c)
				return -1;
			const int r = vips_hip_conva_gen(c, in, &t);
			vips_hip_conva_free(c);
			if (r)
				return -1;
		}
		else {
			ConvRef c(vips_hip_conv_new(plan->masks[k].data(), plan->size, plan->size, plan->scale, plan->offset, plan->precision));
			if (!c.c || vips_hip_conv_gen(c.c, in, &t))
				return -1;
		}
	}
	return compass_combine_run(domain, block.p, (long long) t.stride, (long long) plane, plan->n, plan->times, t.format,
		plan->combine, out->data, (long long) out->stride, (long long) out->width * out->bands, out->height);
}

// vips_compass on a whole image
int vips_hip_compass(VipsHipImage *in, VipsHipImage **out, const double *mask, int mask_width, int mask_height, double scale,
	double offset, int times, int angle, int combine, int precision, int layers, int cluster)
{
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error("compass", "null argument");
		return -1;
	}
	VipsHipCompass *plan = vips_hip_compass_new(mask, mask_width, mask_height, scale, offset, times, angle, combine, precision,
		layers, cluster);
	if (!plan)
		return -1;
	ImageRef o(vips_hip_image_new(in->width, in->height, in->bands, vips_hip_compass_out_format(plan, in->format),
		in->interpretation));
	int r = o.im ? 0 : -1;
	if (!r) {
		VipsHipRegion ri, ro;
		vips_hip_image_region(in, &ri);
		vips_hip_image_region(o.im, &ro);
		r = vips_hip_compass_gen(plan, &ri, &ro);
	}
	vips_hip_compass_free(plan);
	if (r)
		return -1;
	*out = o.release();
	return 0;
}

// ---- vips_canny (convolution/canny.c)

// vips_atan2_init, canny.c:199-223, by its own expression
void vips_hip_canny_table(unsigned char *table)
{
	if (!table)
		return;
	for (int i = 0; i < 256; i++) {
		int x = i & 0xF;
		if (x & 0x8)
			x -= 0x10;
		int y = (i >> 4) & 0xF;
		if (y & 0x8)
			y -= 0x10;
		const double theta = ((atan2(x, y)) / (2.0 * 3.14159265358979323846)) * 360.0 + 360; // VIPS_DEG
		const int value = 256 * theta / 360;
		table[i] = value & 0xFF;
	}
}

// the rows of the BLURRED image behind output rows top .. top + height - 1: one for the thinning's ring and one more
// for the gradient of the ring's upper pels above, the ring's one below
void vips_hip_canny_need(int top, int height, int *in_top, int *in_height)
{
	if (in_top)
		*in_top = top - 2;
	if (in_height)
		*in_height = height + 3;
}

// vips_canny behind its blur: vips_canny_gradient, vips_canny_polar, vips_embed and vips_canny_thin (canny.c:67-378) on
// a window of the blurred image
int vips_hip_canny_gen(const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = "canny";
	if (ensure_init())
		return -1;
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (format_iscomplex(in->format)) {
		error(domain, "complex images are outside the HIP path");
		return -1;
	}
	if (in->format == VIPS_HIP_FORMAT_DOUBLE) {
		error(domain, "double images are outside the HIP path");
		return -1;
	}
	const bool uchar = in->format == VIPS_HIP_FORMAT_UCHAR;
	if (out->format != (uchar ? VIPS_HIP_FORMAT_UCHAR : VIPS_HIP_FORMAT_FLOAT)) {
		error(domain, "the output is uchar for a uchar blur, else float");
		return -1;
	}
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
	int x0 = out->left - 2, x1 = out->left + out->width, y0 = out->top - 2, y1 = out->top + out->height;
	x0 = x0 < 0 ? 0 : x0;
	y0 = y0 < 0 ? 0 : y0;
	x1 = x1 > in->im_width - 1 ? in->im_width - 1 : x1;
	y1 = y1 > in->im_height - 1 ? in->im_height - 1 : y1;
	if (x0 < in->left || y0 < in->top || x1 >= in->left + in->width || y1 >= in->top + in->height) {
		error(domain, "input region too small");
		return -1;
	}
	CannyArgs a = {};
	a.in = (const unsigned char *) in->data;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) out->stride;
	a.in_left = in->left;
	a.in_top = in->top;
	a.in_width = in->width;
	a.in_height = in->height;
	a.im_width = in->im_width;
	a.im_height = in->im_height;
	a.out_left = out->left;
	a.out_top = out->top;
	a.out_width = out->width;
	a.out_height = out->height;
	a.bands = in->bands;
	a.format = in->format;
	unsigned char table[CANNY_TABLE] = { 0 };
	if (uchar)
		vips_hip_canny_table(table);
	else if (!(a.marginal = canny_counter()))
		return -1;
	return canny_run(domain, a, table);
}

// The pels of the float kernel, on the calling thread's device since the last call, whose theta would round to another
// float had atan2's result been 4 ulp off either way; reading clears it.  -1 on error.
long long vips_hip_canny_marginal(void)
{
	if (ensure_init())
		return -1;
	unsigned int *counter = canny_counter();
	if (!counter)
		return -1;
	unsigned int value = 0;
	VH_CHECK(hipMemcpyAsync(&value, counter, sizeof(value), hipMemcpyDeviceToHost, stream()));
	VH_CHECK(hipStreamSynchronize(stream()));
	VH_CHECK(hipMemsetAsync(counter, 0, sizeof(value), stream()));
	return (long long) value;
}

// vips_canny_build, canny.c:380-429
int vips_hip_canny(VipsHipImage *in, VipsHipImage **out, double sigma, int precision)
{
	const char *domain = "canny";
	// decisions hang on the floats (the gradient is a difference of neighbours, thinning keeps or zeroes a pel): the
	// blur reproduces the reference's bits while this runs, whatever the process-wide float mode is
	ScopedExactFloat exact;
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (format_iscomplex(in->format) || in->format == VIPS_HIP_FORMAT_DOUBLE) {
		error(domain, "%s images are outside the HIP path", format_iscomplex(in->format) ? "complex" : "double");
		return -1;
	}
	VipsHipImage *blurred = nullptr;
	if (vips_hip_gaussblur(in, &blurred, sigma, 0.2, precision)) // (min_ampl: the class default, gaussblur.c)
		return -1;
	ImageRef b(blurred);
	const int format = b.im->format == VIPS_HIP_FORMAT_UCHAR ? VIPS_HIP_FORMAT_UCHAR : VIPS_HIP_FORMAT_FLOAT;
	ImageRef o(vips_hip_image_new(b.im->width, b.im->height, b.im->bands, format, in->interpretation));
	if (!o.im)
		return -1;
	VipsHipRegion ri, ro;
	vips_hip_image_region(b.im, &ri);
	vips_hip_image_region(o.im, &ro);
	if (vips_hip_canny_gen(&ri, &ro))
		return -1;
	*out = o.release();
	return 0;
}

} // extern "C"
