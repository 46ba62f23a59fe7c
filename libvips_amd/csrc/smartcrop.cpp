// vips_hist_find (arithmetic/hist_find.c) and vips_smartcrop (conversion/smartcrop.c) on images in HBM: the host
// side.  The kernels are hist.hip (the histograms of up to six rectangles in one launch) and attention.hip (the
// point-wise chain and the arg-max of the attention search); everything else the searches need is an operation
// the library already has.
#include "internal.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace vh;

namespace vh {
// attention.hip
int attention_score(const char *domain, const _VipsHipImage *xyz, const _VipsHipImage *edge, const _VipsHipImage *lab,
	_VipsHipImage *out);
int attention_max(const char *domain, const _VipsHipImage *in, unsigned int *result);
} // namespace vh

namespace {

struct HostBlock {
	void *p;
	explicit HostBlock(size_t size)
		: p(vips_hip_malloc_host(size))
	{
	}
	~HostBlock() { vips_hip_free_host(p); }
};

const char *const mode_names[7] = { "none", "centre", "entropy", "attention", "low", "high", "all" };

// vips_hist_entropy (histogram/hist_entropy.c:61-95) of a UINT histogram image `width` pels wide, one row high,
// whose band-interleaved counters are c[]: the reference's chain of images, an operation at a time.  The
// intermediate images are float, so every step below rounds to float where the reference stores one.
//   vips_avg        a double sum in pel order, divided by the number of values (avg.c:103-105, 137-143)
//   vips_linear1    one constant for every band: the constants are rounded to the OUTPUT type, float, and the
//                   multiply-add is in float (linear.c:213-223)
//   vips_log        log() of the double, 0 for 0, stored as float (math.c:101-108, 156)
//   vips_multiply   float * float
double hist_entropy(const unsigned int *c, int width, int bands)
{
	const int n = width * bands;
	const unsigned long long n_pels = (unsigned long long) width; // (one row)
	double m = 0.0;
	for (int i = 0; i < n; i++)
		m += c[i];
	const unsigned long long vals = n_pels * (unsigned long long) bands;
	double avg = m / vals;
	const double sum = avg * n_pels * bands;
	const float a1 = (float) (1.0 / sum);
	const float a2 = (float) (1.0 / log(2.0));
	m = 0.0;
	for (int i = 0; i < n; i++) {
		const float t0 = a1 * (float) c[i] + 0.0f;
		const float t1 = (float) (t0 == 0.0 ? 0.0 : log((double) t0));
		const float t2 = a2 * t1 + 0.0f;
		const float t3 = t0 * t2;
		m += t3;
	}
	avg = m / vals;
	return -avg * n_pels * bands;
}

int refuse(const char *domain, const VipsHipImage *in, int interesting)
{
	const char *mode = mode_names[interesting];
	if (in->format != VIPS_HIP_FORMAT_UCHAR) {
		error(domain, "crop mode '%s' takes uchar images", mode);
		return -1;
	}
	if (in->bands == 2 || in->bands > 3) {
		error(domain, "crop mode '%s' does not take images with alpha", mode);
		return -1;
	}
	if (interesting == 3 && in->bands != 3) {
		error(domain, "crop mode '%s' takes 3-band images (no B_W to XYZ route)", mode);
		return -1;
	}
	return 0;
}

// vips_smartcrop_entropy, smartcrop.c:106-176.  A round of the reference asks for the left and the right slice,
// decides, then asks for the top and the bottom slice of what is left: six rectangles cover both outcomes, so a
// round here is ONE launch and one copy back.
int entropy_search(const char *domain, VipsHipImage *in, int target_width, int target_height, int *left, int *top)
{
	*left = 0;
	*top = 0;
	int width = in->width, height = in->height;
	const int max_slice_size = (int) fmax(ceil((width - target_width) / 8.0), ceil((height - target_height) / 8.0));
	if (max_slice_size <= 0)
		return 0;
	const int per_hist = 256 * in->bands;
	const int rounds_w = (width - target_width + max_slice_size - 1) / max_slice_size;
	const int rounds_h = (height - target_height + max_slice_size - 1) / max_slice_size;
	const int rounds = rounds_w > rounds_h ? rounds_w : rounds_h;
	const size_t round_bytes = (size_t) HIST_MAX_RECTS * per_hist * sizeof(unsigned int);
	DeviceBlock counters(rounds * round_bytes);
	HostBlock host(round_bytes);
	if (!counters.p || !host.p)
		return -1;
	if (hipMemsetAsync(counters.p, 0, rounds * round_bytes, stream()) != hipSuccess)
		return hip_failed(hipErrorUnknown, "hipMemsetAsync");
	const unsigned int *h = (const unsigned int *) host.p;

	for (int round = 0; width > target_width || height > target_height; round++) {
		const int slice_width = width - target_width < max_slice_size ? width - target_width : max_slice_size;
		const int slice_height = height - target_height < max_slice_size ? height - target_height : max_slice_size;
		const int next_width = width - slice_width;
		// the slices: left, right; top, bottom when the left edge stays; top, bottom when it moves
		HistRect rects[HIST_MAX_RECTS];
		int n = 0, first_v = 0;
		if (slice_width > 0) {
			rects[n++] = { *left, *top, slice_width, height };
			rects[n++] = { *left + width - slice_width, *top, slice_width, height };
		}
		if (slice_height > 0) {
			first_v = n;
			for (int moved = 0; moved <= (slice_width > 0 ? 1 : 0); moved++) {
				const int l = *left + (moved ? slice_width : 0);
				rects[n++] = { l, *top, next_width, slice_height };
				rects[n++] = { l, *top + height - slice_height, next_width, slice_height };
			}
		}
		unsigned int *d = (unsigned int *) counters.p + (size_t) round * HIST_MAX_RECTS * per_hist;
		if (round >= rounds) { // (cannot be: the loop is the reference's, the count is its bound)
			error(domain, "entropy: more rounds than slices");
			return -1;
		}
		if (hist_rects(domain, in, rects, n, d) ||
			vips_hip_memcpy_d2h(host.p, d, (size_t) n * per_hist * sizeof(unsigned int)))
			return -1;

		int moved = 0;
		if (slice_width > 0) {
			const double left_score = hist_entropy(h, 256, in->bands);
			const double right_score = hist_entropy(h + per_hist, 256, in->bands);
			width -= slice_width;
			if (left_score < right_score) {
				*left += slice_width;
				moved = 1;
			}
		}
		if (slice_height > 0) {
			const unsigned int *v = h + (size_t) (first_v + 2 * moved) * per_hist;
			const double top_score = hist_entropy(v, 256, in->bands);
			const double bottom_score = hist_entropy(v + per_hist, 256, in->bands);
			height -= slice_height;
			if (top_score < bottom_score)
				*top += slice_height;
		}
	}
	return 0;
}

// vips_smartcrop_attention, smartcrop.c:204-320
int attention_search(const char *domain, VipsHipImage *in, int target_width, int target_height, int *left, int *top,
	int *attention_x, int *attention_y)
{
	// an arg-max hangs on the floats: the float convolutions reproduce the reference's bits while this runs
	ScopedExactFloat exact;

	const double hscale = 32.0 / in->width;
	const double vscale = 32.0 / in->height;
	double sigma = sqrt(pow(target_width * hscale, 2) + pow(target_height * vscale, 2));
	sigma = sigma / 10 > 1.0 ? sigma / 10 : 1.0;

	static const double edge_mask[9] = { 0.0, -1.0, 0.0, -1.0, 4.0, -1.0, 0.0, -1.0, 0.0 };
	ImageRef small, xyz, edge, lab, blurred;
	// (the edge detector runs on all of XYZ: band 1 of the result is the convolution of band 1)
	if (vips_hip_resize(in, &small.im, hscale, vscale, VIPS_HIP_KERNEL_LANCZOS3, 2.0) ||
		vips_hip_colourspace(small.im, &xyz.im, VIPS_HIP_INTERPRETATION_XYZ) ||
		vips_hip_conv(xyz.im, &edge.im, edge_mask, 3, 3, 1.0, 0.0, VIPS_HIP_PRECISION_INTEGER) ||
		vips_hip_colourspace(xyz.im, &lab.im, VIPS_HIP_INTERPRETATION_LAB)) {
		error(domain, "crop mode 'attention': a step of the search failed");
		return -1;
	}
	ImageRef score(vips_hip_image_new(xyz.im->width, xyz.im->height, 1, VIPS_HIP_FORMAT_FLOAT,
		VIPS_HIP_INTERPRETATION_MULTIBAND));
	DeviceBlock result(3 * sizeof(unsigned int));
	unsigned int found[3];
	if (!score.im || !result.p || attention_score(domain, xyz.im, edge.im, lab.im, score.im) ||
		vips_hip_gaussblur(score.im, &blurred.im, sigma, 0.2, VIPS_HIP_PRECISION_INTEGER) ||
		attention_max(domain, blurred.im, (unsigned int *) result.p) ||
		vips_hip_memcpy_d2h(found, result.p, sizeof(found)))
		return -1;
	if (found[1] == 0xffffffffu) {
		error(domain, "crop mode 'attention': no pel of the score image is a number");
		return -1;
	}

	// smartcrop.c:305-317
	*attention_x = (int) ((int) found[1] / hscale);
	*attention_y = (int) ((int) found[2] / vscale);
	const int l = *attention_x - target_width / 2, t = *attention_y - target_height / 2;
	const int max_l = in->width - target_width, max_t = in->height - target_height;
	*left = l < 0 ? 0 : l > max_l ? max_l : l;
	*top = t < 0 ? 0 : t > max_t ? max_t : t;
	return 0;
}

} // namespace

extern "C" {

int vips_hip_hist_rects(VipsHipImage *in, const int *rects, int n, unsigned int *counts)
{
	const char *domain = "hist_find";
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !rects || !counts) {
		error(domain, "null argument");
		return -1;
	}
	if (n < 1 || n > HIST_MAX_RECTS) {
		error(domain, "1 to %d rectangles a launch", HIST_MAX_RECTS);
		return -1;
	}
	HistRect r[HIST_MAX_RECTS];
	for (int k = 0; k < n; k++)
		r[k] = { rects[4 * k], rects[4 * k + 1], rects[4 * k + 2], rects[4 * k + 3] };
	if (in->format != VIPS_HIP_FORMAT_UCHAR || in->bands < 1 || in->bands > 4) {
		error(domain, "histograms are of uchar images of 1 to 4 bands");
		return -1;
	}
	const size_t bytes = (size_t) n * 256 * in->bands * sizeof(unsigned int);
	DeviceBlock counters(bytes);
	if (!counters.p)
		return -1;
	if (hipMemsetAsync(counters.p, 0, bytes, stream()) != hipSuccess)
		return hip_failed(hipErrorUnknown, "hipMemsetAsync");
	if (hist_rects(domain, in, r, n, (unsigned int *) counters.p) || vips_hip_memcpy_d2h(counts, counters.p, bytes))
		return -1;
	return 0;
}

int vips_hip_hist_find(VipsHipImage *in, VipsHipImage **out, int band)
{
	const char *domain = "hist_find";
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (in->format != VIPS_HIP_FORMAT_UCHAR || in->bands < 1 || in->bands > 4) {
		error(domain, "uchar images of 1 to 4 bands only (format %d, %d bands)", in->format, in->bands);
		return -1;
	}
	if (band < -1 || band >= in->bands) { // vips_check_bandno
		error(domain, "band must be -1, or less than %d", in->bands);
		return -1;
	}
	std::vector<unsigned int> all(256 * (size_t) in->bands);
	const int whole[4] = { 0, 0, in->width, in->height };
	if (vips_hip_hist_rects(in, whole, 1, all.data()))
		return -1;
	// every band: the scan sets mx to 255 (hist_find.c:356-362); one band: the largest value it holds (:332-339)
	int mx = 255;
	std::vector<unsigned int> one;
	const unsigned int *pels = all.data();
	int bands = in->bands;
	if (band >= 0) {
		one.resize(256);
		mx = 0;
		for (int v = 0; v < 256; v++) {
			one[v] = all[(size_t) v * in->bands + band];
			if (one[v])
				mx = v;
		}
		pels = one.data();
		bands = 1;
	}
	*out = vips_hip_image_new_from_memory(pels, mx + 1, 1, bands, VIPS_HIP_FORMAT_UINT, VIPS_HIP_INTERPRETATION_HISTOGRAM);
	return *out ? 0 : -1;
}

int vips_hip_smartcrop(VipsHipImage *in, VipsHipImage **out, int width, int height, int interesting, int *left,
	int *top, int *attention_x, int *attention_y)
{
	const char *domain = "smartcrop";
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (interesting < 0 || interesting > 6) {
		error(domain, "bad crop mode %d", interesting);
		return -1;
	}
	if (width > in->width || height > in->height || width <= 0 || height <= 0) { // smartcrop.c:340-345
		error(domain, "bad extract area");
		return -1;
	}
	int l = 0, t = 0, ax = 0, ay = 0;
	switch (interesting) { // smartcrop.c:359-410
	case 1:
		l = (in->width - width) / 2;
		t = (in->height - height) / 2;
		break;
	case 2:
		if (refuse(domain, in, interesting) || entropy_search(domain, in, width, height, &l, &t))
			return -1;
		break;
	case 3:
		if (refuse(domain, in, interesting) || attention_search(domain, in, width, height, &l, &t, &ax, &ay))
			return -1;
		break;
	case 5:
		l = in->width - width;
		t = in->height - height;
		break;
	case 6:
		width = in->width;
		height = in->height;
		break;
	default: // none, low
		break;
	}
	if (vips_hip_extract_area(in, out, l, t, width, height))
		return -1;
	if (left)
		*left = l;
	if (top)
		*top = t;
	if (attention_x)
		*attention_x = ax;
	if (attention_y)
		*attention_y = ay;
	return 0;
}

} // extern "C"
