// vips_conv, vips_conva, vips_convasep, vips_convsep and vips_gaussblur on images in HBM: the host side.  Each mirrors
// the build() of the corresponding reference class and then runs the region ops once over the whole
// (device-resident) image; the masks' device tables are cached here.
#include "colour.h"
#include "conv.h"

#include <cstring>
#include <list>
#include <memory>
#include <mutex>
#include <vector>

using namespace vh;

namespace {

// Operation cache (the role of iofuncs/cache.c for this path): a mask's device tables are
// built and uploaded once, not per call -- a table upload synchronises the stream, which on a
// 1024^2 thumbnail costs more than the kernels.  LRU, shared_ptr so an eviction cannot pull
// tables out from under a running call; leaked on purpose (no device frees at exit).
typedef std::shared_ptr<VipsHipConv> ConvPtr;

struct ConvKey {
	int device; // a mask's device tables live on one device
	std::vector<double> mask;
	int mw, mh, precision;
	double scale, offset;
	bool operator==(const ConvKey &o) const
	{
		return device == o.device && mw == o.mw && mh == o.mh && precision == o.precision &&
			memcmp(&scale, &o.scale, sizeof(double)) == 0 &&
			memcmp(&offset, &o.offset, sizeof(double)) == 0 && mask.size() == o.mask.size() &&
			memcmp(mask.data(), o.mask.data(), mask.size() * sizeof(double)) == 0;
	}
};

std::mutex &g_conv_mutex = *new std::mutex;
std::list<std::pair<ConvKey, ConvPtr>> &g_conv_cache = *new std::list<std::pair<ConvKey, ConvPtr>>;
const size_t CONV_CACHE_MAX = 64;

ConvPtr conv_cached(const double *mask, int mw, int mh, double scale, double offset, int precision)
{
	if (!mask || mw <= 0 || mh <= 0 || (long long) mw * mh > 65536)
		return ConvPtr(vips_hip_conv_new(mask, mw, mh, scale, offset, precision), vips_hip_conv_free);
	if (ensure_init())
		return ConvPtr();
	ConvKey key = { current_device(), std::vector<double>(mask, mask + (size_t) mw * mh), mw, mh, precision, scale, offset };
	{
		std::lock_guard<std::mutex> lock(g_conv_mutex);
		for (auto it = g_conv_cache.begin(); it != g_conv_cache.end(); ++it)
			if (it->first == key) {
				g_conv_cache.splice(g_conv_cache.begin(), g_conv_cache, it);
				return g_conv_cache.front().second;
			}
	}
	VipsHipConv *raw = vips_hip_conv_new(mask, mw, mh, scale, offset, precision);
	if (!raw)
		return ConvPtr();
	ConvPtr c(raw, vips_hip_conv_free);
	std::lock_guard<std::mutex> lock(g_conv_mutex);
	g_conv_cache.emplace_front(std::move(key), c);
	while (g_conv_cache.size() > CONV_CACHE_MAX)
		g_conv_cache.pop_back();
	return c;
}

// the same for the box / line decompositions of precision=approximate (approx.hip): the
// clustering is host work worth keeping
typedef std::shared_ptr<VipsHipConva> ConvaPtr;

struct ConvaKey {
	ConvKey mask; // precision field: 1 = separable
	int layers, cluster;
	bool operator==(const ConvaKey &o) const { return layers == o.layers && cluster == o.cluster && mask == o.mask; }
};

std::list<std::pair<ConvaKey, ConvaPtr>> &g_conva_cache = *new std::list<std::pair<ConvaKey, ConvaPtr>>;

ConvaPtr conva_cached(const double *mask, int mw, int mh, double scale, double offset, int layers, int cluster,
	bool separable)
{
	auto make = [&]() {
		return separable ? vips_hip_convasep_new(mask, mw * mh, scale, offset, layers)
						 : vips_hip_conva_new(mask, mw, mh, scale, offset, layers, cluster);
	};
	if (!mask || mw <= 0 || mh <= 0 || (long long) mw * mh > 65536)
		return ConvaPtr(make(), vips_hip_conva_free);
	if (ensure_init())
		return ConvaPtr();
	ConvaKey key = { { current_device(), std::vector<double>(mask, mask + (size_t) mw * mh), mw, mh, separable ? 1 : 0, scale, offset },
		layers, cluster };
	{
		std::lock_guard<std::mutex> lock(g_conv_mutex);
		for (auto it = g_conva_cache.begin(); it != g_conva_cache.end(); ++it)
			if (it->first == key) {
				g_conva_cache.splice(g_conva_cache.begin(), g_conva_cache, it);
				return g_conva_cache.front().second;
			}
	}
	VipsHipConva *raw = make();
	if (!raw)
		return ConvaPtr();
	ConvaPtr c(raw, vips_hip_conva_free);
	std::lock_guard<std::mutex> lock(g_conv_mutex);
	g_conva_cache.emplace_front(std::move(key), c);
	while (g_conva_cache.size() > CONV_CACHE_MAX)
		g_conva_cache.pop_back();
	return c;
}

int conv_image(VipsHipImage *in, VipsHipImage **out, const double *mask, int mw, int mh,
	double scale, double offset, int precision)
{
	ConvPtr c = conv_cached(mask, mw, mh, scale, offset, precision);
	if (!c)
		return -1;
	const int fmt = vips_hip_conv_out_format(c.get(), in->format);
	ImageRef o(vips_hip_image_new(in->width, in->height, in->bands, fmt, in->interpretation));
	if (!o.im)
		return -1;
	// uchar, integer precision, a small mask: the packed-byte streaming kernel (conv_u8.hip)
	// (not with the Highway variant of convi selected: that one has its own arithmetic)
	if (in->format == VIPS_HIP_FORMAT_UCHAR && precision == VIPS_HIP_PRECISION_INTEGER && !vips_hip_vector_isenabled() &&
		mh > 1 && mw > 1) {
		int r = vh::conv_u8_mfma_2d_try(in, o.im, c.get()); // the matrix cores first (conv_u8_mfma.hip)
		if (r == 1)
			r = vh::conv_u8_2d_try(in, o.im, c.get());
		if (r < 0)
			return -1;
		if (r == 0) {
			*out = o.release();
			return 0;
		}
	}
	// ushort, integer precision, a mask up to 5 x 5: the streaming kernel on 16-bit lanes (conv_u16.hip)
	if (in->format == VIPS_HIP_FORMAT_USHORT && precision == VIPS_HIP_PRECISION_INTEGER && (mh > 1 || mw > 1)) {
		const int r = vh::conv_u16_2d_try(in, o.im, c.get());
		if (r < 0)
			return -1;
		if (r == 0) {
			*out = o.release();
			return 0;
		}
	}
	VipsHipRegion ri, ro;
	vips_hip_image_region(in, &ri);
	vips_hip_image_region(o.im, &ro);
	if (vips_hip_conv_gen(c.get(), &ri, &ro))
		return -1;
	// the plan's tables go back to the pool behind the kernel on this stream
	*out = o.release();
	return 0;
}

} // namespace

extern "C" {

// vips_conv_build, convolution/conv.c:62-118
int vips_hip_conv(VipsHipImage *in, VipsHipImage **out, const double *mask, int mask_width,
	int mask_height, double scale, double offset, int precision)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out || !mask) {
		error("conv", "null argument");
		return -1;
	}
	// conv.c:99-107 with the class defaults layers = 5, cluster = 1 (:159-160)
	if (precision == VIPS_HIP_PRECISION_APPROXIMATE)
		return vips_hip_conva(in, out, mask, mask_width, mask_height, scale, offset, 5, 1);
	return conv_image(in, out, mask, mask_width, mask_height, scale, offset, precision);
}

// vips_conva_build, convolution/conva.c:1231-1280
int vips_hip_conva(VipsHipImage *in, VipsHipImage **out, const double *mask, int mask_width,
	int mask_height, double scale, double offset, int layers, int cluster)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error("conva", "null argument");
		return -1;
	}
	ConvaPtr c = conva_cached(mask, mask_width, mask_height, scale, offset, layers, cluster, false);
	if (!c)
		return -1;
	ImageRef o(vips_hip_image_new(in->width, in->height, in->bands, in->format, in->interpretation));
	if (!o.im)
		return -1;
	{
		const int r = vh::conva_fast_image(in, o.im, c.get());
		if (r < 0)
			return -1;
		if (r == 0) {
			*out = o.release();
			return 0;
		}
	}
	VipsHipRegion ri, ro;
	vips_hip_image_region(in, &ri);
	vips_hip_image_region(o.im, &ro);
	if (vips_hip_conva_gen(c.get(), &ri, &ro))
		return -1;
	*out = o.release();
	return 0;
}

// vips_convasep_build, convolution/convasep.c:775-828: horizontal pass, then vertical
int vips_hip_convasep(VipsHipImage *in, VipsHipImage **out, const double *mask, int mask_n,
	double scale, double offset, int layers)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error("convasep", "null argument");
		return -1;
	}
	if (mask_n <= 0) {
		error("convasep", "separable matrix images must have width or height 1");
		return -1;
	}
	ConvaPtr c = conva_cached(mask, mask_n, 1, scale, offset, layers, 1, true);
	if (!c)
		return -1;
	ImageRef o(vips_hip_image_new(in->width, in->height, in->bands, in->format, in->interpretation));
	if (!o.im)
		return -1;
	// 8/16-bit images whose sums cannot wrap: both passes in the fused separable kernel
	const int r = vh::convasep_fused(in, o.im, c.get());
	if (r < 0)
		return -1;
	if (r == 0) {
		*out = o.release();
		return 0;
	}
	ImageRef t(vips_hip_image_new(in->width, in->height, in->bands, in->format, in->interpretation));
	if (!t.im)
		return -1;
	VipsHipRegion ri, rt, ro;
	vips_hip_image_region(in, &ri);
	vips_hip_image_region(t.im, &rt);
	vips_hip_image_region(o.im, &ro);
	if (vips_hip_convasep_gen(c.get(), &ri, &rt, 0) || vips_hip_convasep_gen(c.get(), &rt, &ro, 1))
		return -1;
	*out = o.release();
	return 0;
}

// vips_convsep_build, convolution/convsep.c:61-118: conv(M) then conv(rot90(M), offset 0)
int vips_hip_convsep(VipsHipImage *in, VipsHipImage **out, const double *mask, int mask_n,
	double scale, double offset, int precision)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out || !mask) {
		error("convsep", "null argument");
		return -1;
	}
	// convsep.c:81-87 with the class default layers = 5 (:155)
	if (precision == VIPS_HIP_PRECISION_APPROXIMATE)
		return vips_hip_convasep(in, out, mask, mask_n, scale, offset, 5);
	if (mask_n <= 0) {
		error("convsep", "separable matrix images must have width or height 1");
		return -1;
	}
	// float images, and uchar / ushort / short with integer precision: both passes in one
	// streaming kernel (convsep_f32.hip)
	// (with the Highway variant of convi selected, uchar images take the two plain passes)
	const bool vector_uchar = in->format == VIPS_HIP_FORMAT_UCHAR && vips_hip_vector_isenabled();
	if (in->format == VIPS_HIP_FORMAT_FLOAT ||
		(precision == VIPS_HIP_PRECISION_INTEGER && !vector_uchar &&
			(in->format == VIPS_HIP_FORMAT_UCHAR || in->format == VIPS_HIP_FORMAT_USHORT ||
				in->format == VIPS_HIP_FORMAT_SHORT))) {
		ConvPtr c = conv_cached(mask, mask_n, 1, scale, offset, precision);
		if (!c)
			return -1;
		ImageRef o(vips_hip_image_new(in->width, in->height, in->bands, in->format, in->interpretation));
		if (!o.im)
			return -1;
		int r = vh::convsep_stream_fused(in, o.im, c.get(), 0.0, nullptr, 0);
		if (r == 1)
			r = vh::conv_u8_mfma_sep_try(in, o.im, c.get(), 0.0);
		if (r == 1)
			r = vh::conv_u16_mfma_sep_try(in, o.im, c.get(), 0.0);
		if (r == 1)
			r = vh::conv_u8_sep_try(in, o.im, c.get(), 0.0);
		if (r == 1)
			r = vh::convsep_f32_fused(in, o.im, c.get(), 0.0);
		if (r < 0)
			return -1;
		if (r == 0) {
			*out = o.release();
			return 0;
		}
	}
	ImageRef t1;
	// first pass: the mask as given (1 row of mask_n)
	if (conv_image(in, &t1.im, mask, mask_n, 1, scale, offset, precision))
		return -1;
	// second pass: vips_rot(D90) turns the row into a column (same element order
	// top to bottom), same scale, offset forced to 0
	return conv_image(t1.im, out, mask, 1, mask_n, scale, 0.0, precision);
}

// vips_gaussblur_build, convolution/gaussblur.c:71-116
int vips_hip_gaussblur(VipsHipImage *in, VipsHipImage **out, double sigma, double min_ampl,
	int precision)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error("gaussblur", "null argument");
		return -1;
	}
	if (sigma < 0.2) {
		ImageRef o(vips_hip_image_new(in->width, in->height, in->bands, in->format,
			in->interpretation));
		if (!o.im || vips_hip_memcpy_d2d(o.im->data, in->data, in->stride * in->height))
			return -1;
		*out = o.release();
		return 0;
	}
	int width = vips_hip_gaussmat(sigma, min_ampl, 1, precision, nullptr, 0, nullptr);
	if (width < 0)
		return -1;
	std::vector<double> mask(width);
	double scale = 1.0;
	if (vips_hip_gaussmat(sigma, min_ampl, 1, precision, mask.data(), width, &scale) < 0)
		return -1;
	return vips_hip_convsep(in, out, mask.data(), width, scale, 0.0, precision);
}

// vips_gaussblur() followed by vips_colourspace() (gaussblur.c:71-116, colourspace.c:551-612):
// BASELINE config 3.  On a 3-band float image whose route has float colour steps only, both
// convolution passes and the route run in ONE streaming kernel (convsep_stream.hip): the
// blurred image is never written.  Every other case is the two operations, one after the
// other.  The pixels are the same either way.
int vips_hip_gaussblur_colourspace(VipsHipImage *in, VipsHipImage **out, double sigma, double min_ampl,
	int precision, int space)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error("gaussblur", "null argument");
		return -1;
	}
	if (in->format == VIPS_HIP_FORMAT_FLOAT && in->bands == 3 && sigma >= 0.2 &&
		precision != VIPS_HIP_PRECISION_APPROXIMATE) {
		const int interpretation = image_guess_interpretation(in); // gaussblur keeps the interpretation
		const Route *route = route_find(interpretation, space);
		if (route && route->n > 0 && route_is_plain(*route) &&
			step_out_format(route->steps[route->n - 1]) == VIPS_HIP_FORMAT_FLOAT) {
			const int width = vips_hip_gaussmat(sigma, min_ampl, 1, precision, nullptr, 0, nullptr);
			if (width < 0)
				return -1;
			std::vector<double> mask(width);
			double scale = 1.0;
			if (vips_hip_gaussmat(sigma, min_ampl, 1, precision, mask.data(), width, &scale) < 0)
				return -1;
			ConvPtr c = conv_cached(mask.data(), width, 1, scale, 0.0, precision);
			if (!c)
				return -1;
			ImageRef o(vips_hip_image_new(in->width, in->height, 3, VIPS_HIP_FORMAT_FLOAT,
				step_out_interpretation(route->steps[route->n - 1])));
			if (!o.im)
				return -1;
			const int r = vh::convsep_stream_fused(in, o.im, c.get(), 0.0, route->steps, route->n);
			if (r < 0)
				return -1;
			if (r == 0) {
				*out = o.release();
				return 0;
			}
		}
	}
	ImageRef blurred;
	if (vips_hip_gaussblur(in, &blurred.im, sigma, min_ampl, precision))
		return -1;
	return vips_hip_colourspace(blurred.im, out, space);
}

} // extern "C"
