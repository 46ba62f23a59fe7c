// libvips/histogram on images in HBM: vips_maplut, vips_hist_cum, vips_hist_norm, vips_hist_equal, vips_hist_local
// and vips_stdif -- the host side: the reference's argument checks with its messages, the region checks, the small
// histogram arithmetic (256 x bands numbers: host work), the C ABI.  The kernels are hist.hip (maplut_u8) and
// hist_local.hip.
#include "internal.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace vh;

namespace {

const char *format_name(int format)
{
	static const char *names[] = { "uchar", "char", "ushort", "short", "uint", "int", "float", "complex", "double", "dpcomplex" };
	return format >= 0 && format <= 9 ? names[format] : "unknown";
}

// one element of a table: (TYPE) v as the reference's PACK_TABLE stores the identity, maplut.c:562-581
void put_identity(unsigned char *q, int format, int x)
{
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR: { const unsigned char v = (unsigned char) x; memcpy(q, &v, 1); break; }
	case VIPS_HIP_FORMAT_CHAR: { const signed char v = (signed char) x; memcpy(q, &v, 1); break; }
	case VIPS_HIP_FORMAT_USHORT: { const unsigned short v = (unsigned short) x; memcpy(q, &v, 2); break; }
	case VIPS_HIP_FORMAT_SHORT: { const short v = (short) x; memcpy(q, &v, 2); break; }
	case VIPS_HIP_FORMAT_UINT: { const unsigned int v = (unsigned int) x; memcpy(q, &v, 4); break; }
	case VIPS_HIP_FORMAT_INT: { const int v = x; memcpy(q, &v, 4); break; }
	case VIPS_HIP_FORMAT_FLOAT: { const float v = (float) x; memcpy(q, &v, 4); break; }
	default: { const double v = (double) x; memcpy(q, &v, 8); break; }
	}
}

// vips_maplut_build, maplut.c:612-748, on a LUT in host memory: `lut` holds n pels of lut_bands elements
int maplut_apply(const char *domain, VipsHipImage *in, const unsigned char *lut, int n, int lut_bands, int lut_format,
	int lut_interpretation, int band, VipsHipImage **out)
{
	if (in->format != VIPS_HIP_FORMAT_UCHAR) {
		error(domain, "%s index images are outside the HIP path: uchar only", format_name(in->format));
		return -1;
	}
	if (format_iscomplex(lut_format) || format_sizeof(lut_format) == 0) {
		error(domain, "%s tables are outside the HIP path", format_name(lut_format));
		return -1;
	}
	if (n > 256) {
		error(domain, "a table of %d entries: the HIP path indexes with uchar images, tables of up to 256", n);
		return -1;
	}
	if (in->bands != lut_bands && in->bands != 1 && lut_bands != 1) { // vips_check_bands_1orn
		error(domain, "images must have the same number of bands, or one must be single-band");
		return -1;
	}
	const int es = format_sizeof(lut_format);
	const int tables = band >= 0 && lut_bands == 1 ? in->bands : lut_bands; // maplut.c:690-694
	if ((long long) n * tables * es > MAPLUT_TABLE_MAX) {
		error(domain, "a table of %d entries x %d bands of %s: the kernel keeps up to %d bytes", n, tables, format_name(lut_format),
			MAPLUT_TABLE_MAX);
		return -1;
	}
	const size_t table_bytes = ((size_t) n * tables * es + 3) / 4 * 4;
	std::vector<unsigned char> table(table_bytes, 0);
	for (int x = 0; x < n; x++)
		for (int b = 0; b < tables; b++) {
			unsigned char *q = table.data() + ((size_t) x * tables + b) * es;
			if (band >= 0 && lut_bands == 1) {
				if (b == band)
					memcpy(q, lut + (size_t) x * es, es);
				else
					put_identity(q, lut_format, x);
			}
			else
				memcpy(q, lut + ((size_t) x * lut_bands + b) * es, es);
		}

	// maplut.c:648-669
	const int out_bands = lut_bands != 1 ? lut_bands : in->bands;
	const int type = guess_interpretation(lut_bands != 1 ? lut_interpretation : in->interpretation, in->width, in->height, out_bands,
		lut_format);
	ImageRef o(vips_hip_image_new(in->width, in->height, out_bands, lut_format, type));
	if (!o.im)
		return -1;
	// (the block goes back to the pool behind the kernel: the pool hands it out again on this thread's stream only)
	DeviceBlock block(table_bytes);
	if (!block.p || vips_hip_memcpy_h2d(block.p, table.data(), table_bytes))
		return -1;
	MaplutArgs a = {};
	a.in = (const unsigned char *) in->data;
	a.out = (unsigned char *) o.im->data;
	a.table = (const unsigned char *) block.p;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) o.im->stride;
	a.in_elems = in->width * in->bands;
	a.height = in->height;
	a.n = n;
	a.tables = tables;
	a.es = es;
	a.spread = in->bands == 1 && tables > 1 ? tables : 1;
	if ((long long) in->width * in->bands >= (1LL << 31) - 64) {
		error(domain, "image too large");
		return -1;
	}
	if (maplut_run(domain, a))
		return -1;
	*out = o.release();
	return 0;
}

// a one-row UINT histogram in host memory
int fetch_hist(const char *domain, VipsHipImage *in, std::vector<unsigned int> *pels)
{
	if (in->format != VIPS_HIP_FORMAT_UINT || in->height != 1) {
		error(domain, "a %d x %d %s image: histograms here are the one-row uint images of vips_hip_hist_find", in->width, in->height,
			format_name(in->format));
		return -1;
	}
	pels->resize((size_t) in->width * in->bands);
	return vips_hip_image_write_to_memory(in, pels->data());
}

} // namespace

extern "C" {

// ACCUMULATE(unsigned int, unsigned int), hist_cum.c:72-85
void vips_hip_hist_cum_host(const unsigned int *in, int width, int bands, unsigned int *out)
{
	if (!in || !out)
		return;
	for (int b = 0; b < bands; b++) {
		unsigned int total = 0;
		for (int x = 0; x < width; x++) {
			total += in[(size_t) x * bands + b];
			out[(size_t) x * bands + b] = total;
		}
	}
}

// vips_hist_norm_build, hist_norm.c:74-125, step by step
int vips_hip_hist_norm_host(const unsigned int *in, int width, int bands, void *out)
{
	if (!in || !out || width < 1 || bands < 1) {
		error("hist_norm", "null argument");
		return -1;
	}
	// vips_stats: the maximum of each band, a double
	std::vector<double> a(bands);
	const unsigned long long new_max = (unsigned long long) width - 1; // VIPS_IMAGE_N_PELS(in) - 1, :98
	bool single = true; // linear.c:155-179: every a equal (b is 0 throughout)
	for (int b = 0; b < bands; b++) {
		unsigned int mx = 0;
		for (int x = 0; x < width; x++)
			mx = in[(size_t) x * bands + b] > mx ? in[(size_t) x * bands + b] : mx;
		a[b] = new_max / (double) mx; // :104
		single = single && a[b] == a[0];
	}
	const int format = new_max <= 255 ? VIPS_HIP_FORMAT_UCHAR : new_max <= 65535 ? VIPS_HIP_FORMAT_USHORT : VIPS_HIP_FORMAT_UINT; // :111-118
	const double top = format == VIPS_HIP_FORMAT_UCHAR ? 255.0 : format == VIPS_HIP_FORMAT_USHORT ? 65535.0 : 4294967295.0;
	for (int x = 0; x < width; x++)
		for (int b = 0; b < bands; b++) {
			const size_t i = (size_t) x * bands + b;
			float f;
			if (single) { // LOOP1(unsigned int, float), linear.c:213-223: the constants as floats, float arithmetic
				const float a1 = (float) a[0], b1 = (float) 0.0;
				const float product = a1 * (float) in[i];
				f = product + b1;
			}
			else { // LOOPN, :227-235: double constants, stored as a float
				const double product = a[b] * (float) in[i];
				f = (float) (product + 0.0);
			}
			// vips_cast float -> unsigned: CAST_FLOAT_INT, cast.c:231-238: the clip in double, then the C conversion.
			// (A band of zeros divides by zero above and gives a NaN here; the reference's conversion of it is
			// its machine's, this one's is 0.)
			const double d = (double) f;
			const double c = d < 0.0 ? 0.0 : d > top ? top : d;
			const unsigned int v = c == c ? (unsigned int) c : 0u;
			if (format == VIPS_HIP_FORMAT_UCHAR)
				((unsigned char *) out)[i] = (unsigned char) v;
			else if (format == VIPS_HIP_FORMAT_USHORT)
				((unsigned short *) out)[i] = (unsigned short) v;
			else
				((unsigned int *) out)[i] = v;
		}
	return format;
}

int vips_hip_hist_cum(VipsHipImage *in, VipsHipImage **out)
{
	const char *domain = "hist_cum";
	if (in && bind_to(in))
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	std::vector<unsigned int> pels;
	if (fetch_hist(domain, in, &pels))
		return -1;
	std::vector<unsigned int> cum(pels.size());
	vips_hip_hist_cum_host(pels.data(), in->width, in->bands, cum.data());
	*out = vips_hip_image_new_from_memory(cum.data(), in->width, 1, in->bands, VIPS_HIP_FORMAT_UINT, VIPS_HIP_INTERPRETATION_HISTOGRAM);
	return *out ? 0 : -1;
}

int vips_hip_hist_norm(VipsHipImage *in, VipsHipImage **out)
{
	const char *domain = "hist_norm";
	if (in && bind_to(in))
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	std::vector<unsigned int> pels;
	if (fetch_hist(domain, in, &pels))
		return -1;
	std::vector<unsigned int> norm(pels.size());
	const int format = vips_hip_hist_norm_host(pels.data(), in->width, in->bands, norm.data());
	*out = vips_hip_image_new_from_memory(norm.data(), in->width, 1, in->bands, format, VIPS_HIP_INTERPRETATION_HISTOGRAM);
	return *out ? 0 : -1;
}

int vips_hip_maplut(VipsHipImage *in, VipsHipImage *lut, VipsHipImage **out, int band)
{
	const char *domain = "maplut";
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !lut || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (lut->width != 1 && lut->height != 1) { // vips_check_hist
		error(domain, "histograms must have width or height 1");
		return -1;
	}
	if ((long long) lut->width * lut->height > 65536) {
		error(domain, "histograms must have not have more than 65536 elements");
		return -1;
	}
	const int n = lut->width * lut->height;
	if (n > 256) {
		error(domain, "a table of %d entries: the HIP path indexes with uchar images, tables of up to 256", n);
		return -1;
	}
	std::vector<unsigned char> pels(lut->stride * lut->height);
	if (vips_hip_image_write_to_memory(lut, pels.data()) || bind_to(in))
		return -1;
	return maplut_apply(domain, in, pels.data(), n, lut->bands, lut->format, lut->interpretation, band, out);
}

// vips_hist_equal_build, hist_equal.c:74-98: hist_find(band) -> cum -> norm -> cast to the input's format -> maplut
int vips_hip_hist_equal(VipsHipImage *in, VipsHipImage **out, int band)
{
	const char *domain = "hist_equal";
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (in->format != VIPS_HIP_FORMAT_UCHAR || in->bands < 1 || in->bands > 4) {
		error(domain, "%s images of %d bands are outside the HIP path: uchar of 1 to 4 bands", format_name(in->format), in->bands);
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
	// as vips_hip_hist_find: every band, 256 wide; one band, as wide as the largest value it holds + 1
	int width = 256, bands = in->bands;
	std::vector<unsigned int> hist;
	if (band >= 0) {
		int mx = 0;
		for (int v = 0; v < 256; v++)
			if (all[(size_t) v * in->bands + band])
				mx = v;
		width = mx + 1;
		bands = 1;
		hist.resize(width);
		for (int v = 0; v < width; v++)
			hist[v] = all[(size_t) v * in->bands + band];
	}
	else
		hist = all;
	std::vector<unsigned int> cum(hist.size());
	vips_hip_hist_cum_host(hist.data(), width, bands, cum.data());
	// a histogram is at most 256 wide: the normalised one is uchar, the cast to the input's format changes nothing
	std::vector<unsigned char> lut(hist.size());
	if (vips_hip_hist_norm_host(cum.data(), width, bands, lut.data()) != VIPS_HIP_FORMAT_UCHAR) {
		error(domain, "normalised histogram is not uchar");
		return -1;
	}
	return maplut_apply(domain, in, lut.data(), width, bands, VIPS_HIP_FORMAT_UCHAR, VIPS_HIP_INTERPRETATION_HISTOGRAM, -1, out);
}

// ---- hist_local, stdif

// the checks hist_local and stdif share: vips_check_format uchar, the window against the whole image
static int window_checks(const char *domain, const VipsHipRegion *in, const VipsHipRegion *out, int width, int height)
{
	if (ensure_init())
		return -1;
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (in->format != VIPS_HIP_FORMAT_UCHAR) { // vips_check_format's words, and which format it was
		error(domain, "image must be VIPS_FORMAT_UCHAR (it is %s)", format_name(in->format));
		return -1;
	}
	if (width < 1 || height < 1 || width > in->im_width || height > in->im_height) {
		error(domain, "window too large");
		return -1;
	}
	if (out->format != VIPS_HIP_FORMAT_UCHAR) {
		error(domain, "output region has the wrong format");
		return -1;
	}
	return 0;
}

// vips_hist_local_generate, hist_local.c:142-270, with the checks of vips_hist_local_build :286-297
int vips_hip_hist_local_gen(const VipsHipRegion *in, const VipsHipRegion *out, int width, int height, int max_slope)
{
	const char *domain = "hist_local";
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (window_checks(domain, in, out, width, height))
		return -1;
	if (max_slope < 0 || max_slope > 100) {
		error(domain, "max_slope must be 0 to 100");
		return -1;
	}
	NbArgs a;
	if (nb_geometry(domain, in, out, width, height, &a))
		return -1;
	return hist_local_run(domain, a, max_slope);
}

int vips_hip_hist_local_step(int what)
{
	return hist_local_tile(what);
}

int vips_hip_hist_local(VipsHipImage *in, VipsHipImage **out, int width, int height, int max_slope)
{
	if (enter("hist_local", in, out))
		return -1;
	return whole_image(in, out, in->bands, VIPS_HIP_FORMAT_UCHAR,
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_hist_local_gen(ri, ro, width, height, max_slope); });
}

// vips_stdif_generate, stdif.c:135-253, with the checks of vips_stdif_build :273-280
int vips_hip_stdif_gen(const VipsHipRegion *in, const VipsHipRegion *out, int width, int height, double a, double m0, double b,
	double s0)
{
	const char *domain = "stdif";
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (window_checks(domain, in, out, width, height))
		return -1;
	StdifArgs sa = {};
	if (nb_geometry(domain, in, out, width, height, &sa.nb))
		return -1;
	// stdif.c:170-172
	sa.f1 = a * m0;
	sa.f2 = 1.0 - a;
	sa.f3 = b * s0;
	sa.s0 = s0;
	sa.b = b;
	return stdif_run(domain, sa);
}

int vips_hip_stdif_step(int what)
{
	return stdif_tile(what);
}

int vips_hip_stdif(VipsHipImage *in, VipsHipImage **out, int width, int height, double a, double m0, double b, double s0)
{
	if (enter("stdif", in, out))
		return -1;
	return whole_image(in, out, in->bands, VIPS_HIP_FORMAT_UCHAR,
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_stdif_gen(ri, ro, width, height, a, m0, b, s0); });
}

} // extern "C"
