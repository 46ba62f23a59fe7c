// vips_fastcor and vips_spcor (convolution/correlation.c, fastcor.c, spcor.c) on images in HBM: the host side -- the
// build of vips_correlation_build (the header, vips__formatalike and vips__bandalike through what vips_add uses, the
// refusals), the per-band constants of vips_spcor_pre_generate on a host copy of the ref, the C ABI.  The kernels are
// in correlation.hip.
#include "internal.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace vh;

static_assert(VIPS_HIP_CORRELATION_MAX_SIDE >= 64, "the least the ABI promises");

namespace {

struct CorPlan {
	const char *domain;
	int spcor;
};

// correlation.c:98-118: the common format and bands, the size of `in`, the interpretation of the matched `in`, the format tables of
// fastcor.c:206-209 and spcor.c:305-308
int cor_plan(const void *closure, const VipsHipImage *in, const VipsHipImage *ref, BinaryOperands *b)
{
	const CorPlan *plan = (const CorPlan *) closure;
	const char *domain = plan->domain;
	if (in->width < 1 || in->height < 1 || in->bands < 1 || ref->width < 1 || ref->height < 1 || ref->bands < 1) {
		error(domain, "bad image size");
		return -1;
	}
	if (arithmetic_noncomplex(domain, in->format) || arithmetic_noncomplex(domain, ref->format))
		return -1;
	// vips__bandalike_vec, arithmetic.c:210-254
	const int n = in->bands > ref->bands ? in->bands : ref->bands;
	if ((in->bands != n && in->bands != 1) || (ref->bands != n && ref->bands != 1)) {
		error(domain, "not one band or %d bands", n);
		return -1;
	}
	const int limit = correlation_tile(2);
	if (ref->width > limit || ref->height > limit) {
		error(domain, "a %d x %d ref is outside the HIP path (refs up to %d x %d)", ref->width, ref->height, limit, limit);
		return -1;
	}
	b->format = format_common(in->format, ref->format);
	if (plan->spcor)
		b->out_format = VIPS_HIP_FORMAT_FLOAT;
	else
		b->out_format = format_isint(b->format) ? VIPS_HIP_FORMAT_UINT : b->format;
	b->bands = n;
	// the header is in_ready's: the image's own interpretation, or, banded up, that of the ref it was matched to
	b->interpretation = in->bands == n ? in->interpretation : ref->interpretation;
	b->width = in->width;
	b->height = in->height;
	return 0;
}

template <typename T>
double element_of(const unsigned char *row, int i)
{
	return (double) ((const T *) row)[i];
}

double element(const unsigned char *row, int i, int format)
{
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR: return element_of<unsigned char>(row, i);
	case VIPS_HIP_FORMAT_CHAR: return element_of<signed char>(row, i);
	case VIPS_HIP_FORMAT_USHORT: return element_of<unsigned short>(row, i);
	case VIPS_HIP_FORMAT_SHORT: return element_of<short>(row, i);
	case VIPS_HIP_FORMAT_UINT: return element_of<unsigned int>(row, i);
	case VIPS_HIP_FORMAT_INT: return element_of<int>(row, i);
	case VIPS_HIP_FORMAT_FLOAT: return element_of<float>(row, i);
	default: return element_of<double>(row, i);
	}
}

int correlation_image(int spcor, VipsHipImage *in, VipsHipImage *ref, VipsHipImage **out)
{
	const char *domain = spcor ? "spcor" : "fastcor";
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !ref || !out) {
		error(domain, "null argument");
		return -1;
	}
	const CorPlan plan = { domain, spcor };
	BinaryOperands b;
	if (binary_operands(domain, in, ref, cor_plan, &plan, &b))
		return -1;
	const VipsHipImage *im = b.cast[0].im ? b.cast[0].im : in;
	const VipsHipImage *rf = b.cast[1].im ? b.cast[1].im : ref;

	CorrelationArgs a;
	memset(&a, 0, sizeof(a));
	a.in = (const unsigned char *) im->data;
	a.ref = (const unsigned char *) rf->data;
	a.out = (unsigned char *) b.out.im->data;
	a.in_stride = (long long) im->stride;
	a.ref_stride = (long long) rf->stride;
	a.out_stride = (long long) b.out.im->stride;
	a.width = im->width;
	a.height = im->height;
	a.in_bands = im->bands;
	a.ref_bands = rf->bands;
	a.bands = b.bands;
	a.ref_w = rf->width;
	a.ref_h = rf->height;
	if (!spcor) {
		if (correlation_run(domain, a, b.format, 0))
			return -1;
		*out = b.out.release();
		return 0;
	}

	// spcor.c:99-152 on a host copy of the ref: it is small
	const size_t row_bytes = (size_t) rf->width * rf->bands * format_sizeof(b.format);
	const size_t n = (size_t) rf->width * rf->height;
	std::vector<unsigned char> host((size_t) (rf->height - 1) * rf->stride + row_bytes);
	if (vips_hip_memcpy_d2h(host.data(), rf->data, host.size()))
		return -1;
	std::vector<double> rmean(b.bands), c1(b.bands), table(n * b.bands);
	if (vips_hip_spcor_constants(host.data(), rf->width, rf->height, rf->bands, b.format, rf->stride, b.bands, rmean.data(), c1.data()))
		return -1;
	// (rp - spcor->rmean[b]), spcor.c:195
	for (int band = 0; band < b.bands; band++) {
		const int rb = rf->bands == 1 ? 0 : band;
		for (int y = 0; y < rf->height; y++)
			for (int x = 0; x < rf->width; x++)
				table[(size_t) band * n + (size_t) y * rf->width + x] =
					element(host.data() + (size_t) y * rf->stride, x * rf->bands + rb, b.format) - rmean[band];
	}
	DeviceBlock dtable(table.size() * sizeof(double)), dc1(c1.size() * sizeof(double));
	if (!dtable.p || !dc1.p)
		return -1;
	if (vips_hip_memcpy_h2d(dtable.p, table.data(), table.size() * sizeof(double)) ||
		vips_hip_memcpy_h2d(dc1.p, c1.data(), c1.size() * sizeof(double)))
		return -1;
	a.table = (const double *) dtable.p;
	a.c1 = (const double *) dc1.p;
	if (correlation_run(domain, a, b.format, 1))
		return -1;
	// (the blocks go back to the pool behind the kernel: the pool hands them out again on this thread's stream only)
	*out = b.out.release();
	return 0;
}

} // namespace

extern "C" {

int vips_hip_spcor_constants(const void *pixels, int width, int height, int bands, int format, size_t stride, int out_bands,
	double *rmean, double *c1)
{
	const char *domain = "spcor";
	if (!pixels || !rmean || !c1 || width < 1 || height < 1 || bands < 1 || out_bands < 1) {
		error(domain, "bad arguments");
		return -1;
	}
	if (arithmetic_noncomplex(domain, format))
		return -1;
	if (bands != out_bands && bands != 1) {
		error(domain, "not one band or %d bands", out_bands);
		return -1;
	}
	const unsigned char *base = (const unsigned char *) pixels;
	// vips_avg (avg.c:103-105, :157-210) of every band: a double sum in raster order over the band's elements
	const double vals = (double) ((unsigned long long) width * (unsigned long long) height);
	for (int b = 0; b < out_bands; b++) {
		const int rb = bands == 1 ? 0 : b;
		double sum = 0.0;
		for (int y = 0; y < height; y++)
			for (int x = 0; x < width; x++)
				sum += element(base + (size_t) y * stride, x * bands + rb, format);
		rmean[b] = sum / vals;
	}
	// linear.c:155-179: offsets that are all equal count as one, and LOOP1 runs (linear.c:213-223)
	bool single = true;
	for (int b = 1; b < out_bands; b++)
		if (-rmean[b] != -rmean[0])
			single = false;
	// spcor.c:146-148: c1 *= Xsize * Ysize, an int
	const double count = (double) (width * height);
	for (int b = 0; b < out_bands; b++) {
		const int rb = bands == 1 ? 0 : b;
		const double offset = -rmean[b];
		double sum = 0.0;
		for (int y = 0; y < height; y++)
			for (int x = 0; x < width; x++) {
				const unsigned char *row = base + (size_t) y * stride;
				const int i = x * bands + rb;
				if (format == VIPS_HIP_FORMAT_DOUBLE) {
					// linear, multiply and avg all stay double
					const double v = 1.0 * element(row, i, format) + offset;
					sum += v * v;
				}
				else {
					// (OUT) p[x]: the element as a float
					const float p = (float) element(row, i, format); // (every integer is exact in the double: rounded once)
					float v;
					if (single) {
						const float a1 = 1.0f, b1 = (float) -rmean[0];
						v = a1 * p + b1;
					}
					else
						v = (float) (1.0 * (double) p + offset); // LOOPN: a[k] and b[k] are doubles
					const float sq = v * v; // vips_multiply of float images
					sum += (double) sq;
				}
			}
		c1[b] = sqrt((sum / vals) * count);
	}
	return 0;
}

int vips_hip_fastcor(VipsHipImage *in, VipsHipImage *ref, VipsHipImage **out)
{
	return correlation_image(0, in, ref, out);
}

int vips_hip_spcor(VipsHipImage *in, VipsHipImage *ref, VipsHipImage **out)
{
	return correlation_image(1, in, ref, out);
}

int vips_hip_correlation_step(int what)
{
	return correlation_tile(what);
}

} // extern "C"
