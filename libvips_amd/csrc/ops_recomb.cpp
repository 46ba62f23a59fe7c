// vips_recomb (conversion/recomb.c) on images in HBM: the host side -- vips_recomb_build restated (its checks in its
// order and words, the output's bands and format), the matrix turned to doubles as vips_check_matrix turns it, the
// region checks, the C ABI.  The kernels are in recomb.hip.
#include "internal.h"

#include <cstring>
#include <vector>

using namespace vh;

static_assert(RECOMB_MAX == VIPS_HIP_ARITH_MAX_VECTOR, "one limit for what multiplies a pel's bands");

namespace {

const char *const DOMAIN = "recomb";

// vips_cast to double of one element of a real format: exact
double element_of(const unsigned char *p, int format)
{
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR: return *p;
	case VIPS_HIP_FORMAT_CHAR: return *(const signed char *) p;
#define AS(T) \
	{ \
		T v; \
		memcpy(&v, p, sizeof(v)); \
		return (double) v; \
	}
	case VIPS_HIP_FORMAT_USHORT: AS(unsigned short)
	case VIPS_HIP_FORMAT_SHORT: AS(short)
	case VIPS_HIP_FORMAT_UINT: AS(unsigned int)
	case VIPS_HIP_FORMAT_INT: AS(int)
	case VIPS_HIP_FORMAT_FLOAT: AS(float)
	default: AS(double)
#undef AS
	}
}

} // namespace

extern "C" {

int vips_hip_recomb_plan(int bands, int format, int mwidth, int mheight, int m_bands, int m_format, int *out_bands, int *out_format)
{
	if (!out_bands || !out_format || bands < 1 || mwidth < 1 || mheight < 1) {
		error(DOMAIN, "bad arguments");
		return -1;
	}
	// recomb.c:174-185
	if (arithmetic_noncomplex(DOMAIN, format) || arithmetic_noncomplex(DOMAIN, m_format))
		return -1;
	if (m_bands != 1) {
		error(DOMAIN, "image must one band");
		return -1;
	}
	if (bands != mwidth) {
		error(DOMAIN, "bands in must equal matrix width");
		return -1;
	}
	if (mwidth > RECOMB_MAX || mheight > RECOMB_MAX) {
		error(DOMAIN, "a matrix of %d x %d is outside the HIP path (at most %d x %d)", mwidth, mheight, RECOMB_MAX, RECOMB_MAX);
		return -1;
	}
	// recomb.c:195-197
	*out_bands = mheight;
	*out_format = format <= VIPS_HIP_FORMAT_INT ? VIPS_HIP_FORMAT_FLOAT : format;
	return 0;
}

int vips_hip_recomb_gen(const double *m, int mwidth, int mheight, const VipsHipRegion *in, const VipsHipRegion *out)
{
	if (ensure_init())
		return -1;
	if (arithmetic_window_pair(DOMAIN, in, out))
		return -1;
	if (!m) {
		error(DOMAIN, "null argument");
		return -1;
	}
	int bands, format;
	if (vips_hip_recomb_plan(in->bands, in->format, mwidth, mheight, 1, VIPS_HIP_FORMAT_DOUBLE, &bands, &format))
		return -1;
	if (out->bands != bands || out->format != format) {
		error(DOMAIN, "the output must have %d bands of format %d", bands, format);
		return -1;
	}
	RecombArgs a;
	memset(&a, 0, sizeof(a));
	a.in = (const unsigned char *) in->data;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) out->stride;
	a.width = out->width;
	a.height = out->height;
	a.mwidth = mwidth;
	a.mheight = mheight;
	return recomb_run(DOMAIN, in->format, a, m);
}

int vips_hip_recomb_matrix(VipsHipImage *in, VipsHipImage **out, const double *m, int mwidth, int mheight)
{
	if (enter(DOMAIN, in, out))
		return -1;
	if (!m) {
		error(DOMAIN, "null argument");
		return -1;
	}
	int bands, format;
	if (vips_hip_recomb_plan(in->bands, in->format, mwidth, mheight, 1, VIPS_HIP_FORMAT_DOUBLE, &bands, &format))
		return -1;
	return whole_image(in, out, bands, format,
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_recomb_gen(m, mwidth, mheight, ri, ro); });
}

int vips_hip_recomb(VipsHipImage *in, VipsHipImage **out, VipsHipImage *m)
{
	if (enter(DOMAIN, in, out))
		return -1;
	if (!m) {
		error(DOMAIN, "null argument");
		return -1;
	}
	// (before anything is downloaded: a matrix that is refused is refused by its header)
	int bands, format;
	if (vips_hip_recomb_plan(in->bands, in->format, m->width, m->height, m->bands, m->format, &bands, &format))
		return -1;
	// vips_check_matrix, iofuncs/error.c:1196-1222: the matrix as doubles in host memory
	std::vector<unsigned char> raw(m->stride * (size_t) m->height);
	if (vips_hip_image_write_to_memory(m, raw.data()) || bind_to(in))
		return -1;
	std::vector<double> coeff((size_t) m->width * m->height);
	const int es = format_sizeof(m->format);
	for (int y = 0; y < m->height; y++)
		for (int x = 0; x < m->width; x++)
			coeff[(size_t) y * m->width + x] = element_of(raw.data() + (size_t) y * m->stride + (size_t) x * es, m->format);
	return vips_hip_recomb_matrix(in, out, coeff.data(), m->width, m->height);
}

int vips_hip_recomb_step(int what)
{
	return recomb_tile(what);
}

} // extern "C"
