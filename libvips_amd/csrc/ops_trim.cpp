// vips_project, vips_profile, vips_getpoint and vips_find_trim (arithmetic/project.c, profile.c, getpoint.c, find_trim.c)
// on images in HBM: the host side -- each build() restated (the format table, the outputs' headers, the errors with the
// reference's words), find_trim's two routes, its predicate table and its finish, the C ABI.  The kernels are in
// trim.hip.
#include "internal.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace vh;

static_assert(VIPS_HIP_TRIM_MAX_BACKGROUND == VIPS_HIP_ARITH_MAX_VECTOR, "the background is vips_linear's b");

namespace {

int enter(const char *domain, VipsHipImage *in, const void *out1, const void *out2)
{
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out1 || !out2) {
		error(domain, "null argument");
		return -1;
	}
	return 0;
}

// the two outputs of project and profile (project.c:154-166, profile.c:139-149)
int outputs(const VipsHipImage *in, int format, ImageRef *columns, ImageRef *rows)
{
	columns->im = vips_hip_image_new(in->width, 1, in->bands, format, VIPS_HIP_INTERPRETATION_HISTOGRAM);
	rows->im = vips_hip_image_new(1, in->height, in->bands, format, VIPS_HIP_INTERPRETATION_HISTOGRAM);
	return columns->im && rows->im ? 0 : -1;
}

bool hasalpha(const VipsHipImage *im)
{
	const int bands = interpretation_bands(im->interpretation);
	return bands > 0 && im->bands > bands;
}

// the arguments with the defaults filled in: find_trim.c:95-97, and a threshold the property refuses
void settle(const VipsHipFindTrim *args, int interpretation, VipsHipFindTrim *out)
{
	vips_hip_find_trim_defaults(out);
	if (args) {
		if (args->threshold >= 0.0)
			out->threshold = args->threshold;
		out->line_art = args->line_art;
		out->n_background = args->n_background;
		for (int i = 0; i < args->n_background && i < VIPS_HIP_TRIM_MAX_BACKGROUND; i++)
			out->background[i] = args->background[i];
	}
	if (out->n_background < 1) {
		out->n_background = 1;
		out->background[0] = vips_hip_find_trim_background(interpretation);
	}
}

int check_args(const char *domain, const VipsHipFindTrim *args)
{
	if (args && (args->n_background < 0 || args->n_background > VIPS_HIP_TRIM_MAX_BACKGROUND)) {
		error(domain, "background of more than %d elements", VIPS_HIP_TRIM_MAX_BACKGROUND);
		return -1;
	}
	return 0;
}

// find_trim.c:112-119, :131: vips_linear(in, ones, neg_bg, n)
void linear_args(const VipsHipFindTrim &s, VipsHipLinear *l)
{
	vips_hip_linear_defaults(l);
	l->n_a = l->n_b = s.n_background;
	for (int i = 0; i < s.n_background; i++) {
		l->a[i] = 1.0;
		l->b[i] = -1 * s.background[i];
	}
}

// find_trim.c:123-141 on the flattened image, with this library's own operations; the sums come back to the host in
// one copy
int composed(VipsHipImage *in, const VipsHipFindTrim &s, int *left, int *top, int *width, int *height)
{
	ImageRef t[6], columns, rows;
	VipsHipImage *cur = in;
	if (!s.line_art) {
		if (vips_hip_median(cur, &t[0].im, 3))
			return -1;
		cur = t[0].im;
	}
	VipsHipLinear l;
	linear_args(s, &l);
	const double threshold = s.threshold;
	if (vips_hip_linear(cur, &t[1].im, &l) || vips_hip_abs(t[1].im, &t[2].im) ||
		vips_hip_relational_const(t[2].im, &t[3].im, VIPS_HIP_RELATIONAL_MORE, &threshold, 1) ||
		vips_hip_bandbool(t[3].im, &t[4].im, VIPS_HIP_BOOLEAN_OR) || vips_hip_project(t[4].im, &columns.im, &rows.im))
		return -1;
	// (more_const gives uchar whatever it is given, so the sums are uint: relational.c:214-217, project.c:99-102)
	if (columns.im->format != VIPS_HIP_FORMAT_UINT || columns.im->bands != 1) {
		error("find_trim", "unexpected projection");
		return -1;
	}
	// the two projections lie in two pool blocks: one staging block, one copy to the host
	const size_t nc = (size_t) columns.im->width, nr = (size_t) rows.im->height;
	DeviceBlock both((nc + nr) * sizeof(unsigned int));
	if (!both.p)
		return -1;
	std::vector<unsigned int> sums(nc + nr);
	if (vips_hip_memcpy_d2d(both.p, columns.im->data, nc * sizeof(unsigned int)) ||
		vips_hip_memcpy_d2d((unsigned int *) both.p + nc, rows.im->data, nr * sizeof(unsigned int)) ||
		vips_hip_memcpy_d2h(sums.data(), both.p, (nc + nr) * sizeof(unsigned int)))
		return -1;
	return vips_hip_find_trim_finish(sums.data(), (int) nc, sums.data() + nc, (int) nr, left, top, width, height);
}

constexpr int TABLE_BYTES = 256 * 4;

int fused(VipsHipImage *in, const VipsHipFindTrim &s, const unsigned char *table, int *left, int *top, int *width, int *height)
{
	const char *domain = "find_trim";
	// the table and the four zero bounds behind it: one block, one copy
	unsigned char host[TABLE_BYTES + 16];
	memset(host, 0, sizeof(host));
	memcpy(host, table, (size_t) 256 * in->bands);
	DeviceBlock block(sizeof(host));
	if (!block.p)
		return -1;
	unsigned int bounds[4];
	if (vips_hip_memcpy_h2d_async(block.p, host, sizeof(host)) ||
		trim_fused_run(domain, in, !s.line_art, (const unsigned char *) block.p, (unsigned int *) ((unsigned char *) block.p + TABLE_BYTES)) ||
		vips_hip_memcpy_d2h(bounds, (unsigned char *) block.p + TABLE_BYTES, sizeof(bounds)))
		return -1;
	// bounds: width - min x, max x + 1, height - min y, max y + 1; 0: nothing set.  The reference's left is the first
	// non-zero column sum, a column sum is non-zero where a pel of the column is set, so left = min x; its `right` is
	// the first non-zero sum of the flipped columns, width - 1 - max x, so its width, (Xsize - right) - left, is
	// max x + 1 - min x.  With nothing set both profiles give Xsize: left = Xsize and VIPS_MAX(0, -Xsize) = 0.
	if (!bounds[1]) {
		*left = in->width;
		*top = in->height;
		*width = *height = 0;
		return 0;
	}
	*left = in->width - (int) bounds[0];
	*width = (int) bounds[1] - *left;
	*top = in->height - (int) bounds[2];
	*height = (int) bounds[3] - *top;
	return 0;
}

template <typename T>
double element(const unsigned char *p, int i)
{
	T v;
	memcpy(&v, p + (size_t) i * sizeof(T), sizeof(T));
	return (double) v;
}

} // namespace

extern "C" {

int vips_hip_project_format(int format)
{
	enum { UI = VIPS_HIP_FORMAT_UINT, I = VIPS_HIP_FORMAT_INT, D = VIPS_HIP_FORMAT_DOUBLE, N = -1 };
	// project.c:99-102
	static const int table[10] = { UI, I, UI, I, UI, I, D, N, D, N };
	if (format < 0 || format > VIPS_HIP_FORMAT_DPCOMPLEX)
		return -1;
	return table[format];
}

int vips_hip_project(VipsHipImage *in, VipsHipImage **columns, VipsHipImage **rows)
{
	const char *domain = "project";
	if (enter(domain, in, columns, rows))
		return -1;
	if (arithmetic_noncomplex(domain, in->format)) // project.c:137-139
		return -1;
	const int format = vips_hip_project_format(in->format);
	ImageRef c, r;
	if (outputs(in, format, &c, &r))
		return -1;
	if (format != VIPS_HIP_FORMAT_DOUBLE) {
		VH_CHECK(hipMemsetAsync(c.im->data, 0, c.im->stride, stream()));
		VH_CHECK(hipMemsetAsync(r.im->data, 0, r.im->stride * r.im->height, stream()));
		if (project_run(domain, in, c.im->data, r.im->data, nullptr, nullptr, nullptr))
			return -1;
	}
	else {
		int grid[3];
		project_grid(in, grid);
		const size_t elems = (size_t) in->width * in->bands, n_rows = (size_t) in->height * in->bands;
		const size_t col_part = (size_t) grid[1] * elems, row_part = (size_t) grid[0] * n_rows;
		// (the block goes back to the pool behind the kernel: the pool hands it out again on this thread's stream only)
		DeviceBlock slab((col_part + row_part + 1) * sizeof(double));
		if (!slab.p)
			return -1;
		double *base = (double *) slab.p;
		unsigned int *ticket = (unsigned int *) (base + col_part + row_part);
		VH_CHECK(hipMemsetAsync(ticket, 0, sizeof(double), stream()));
		if (project_run(domain, in, c.im->data, r.im->data, base, base + col_part, ticket))
			return -1;
	}
	*columns = c.release();
	*rows = r.release();
	return 0;
}

int vips_hip_profile(VipsHipImage *in, VipsHipImage **columns, VipsHipImage **rows)
{
	const char *domain = "profile";
	if (enter(domain, in, columns, rows))
		return -1;
	if (arithmetic_noncomplex(domain, in->format)) // profile.c:122-124
		return -1;
	ImageRef c, r;
	if (outputs(in, VIPS_HIP_FORMAT_INT, &c, &r))
		return -1;
	// edges_new, profile.c:105-108
	const size_t nc = (size_t) in->width * in->bands, nr = (size_t) in->height * in->bands;
	std::vector<int> fill(nc > nr ? nc : nr);
	for (size_t i = 0; i < nc; i++)
		fill[i] = in->height;
	if (vips_hip_memcpy_h2d(c.im->data, fill.data(), nc * sizeof(int)))
		return -1;
	for (size_t i = 0; i < nr; i++)
		fill[i] = in->width;
	if (vips_hip_memcpy_h2d(r.im->data, fill.data(), nr * sizeof(int)))
		return -1;
	if (profile_run(domain, in, (int *) c.im->data, (int *) r.im->data))
		return -1;
	*columns = c.release();
	*rows = r.release();
	return 0;
}

int vips_hip_getpoint(VipsHipImage *in, int x, int y, double *out, int n)
{
	const char *domain = "getpoint";
	if (in && bind_to(in))
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	// vips_crop(in, x, y, 1, 1), getpoint.c:113, extract.c's check
	if (x < 0 || y < 0 || (long long) x + 1 > in->width || (long long) y + 1 > in->height) {
		error("extract_area", "bad extract area");
		return -1;
	}
	if (format_iscomplex(in->format) || format_sizeof(in->format) == 0) {
		error(domain, "complex images are outside the HIP path");
		return -1;
	}
	if (n < in->bands) {
		error(domain, "the output takes %d values", in->bands);
		return -1;
	}
	const size_t es = (size_t) format_sizeof(in->format), pel = es * in->bands;
	std::vector<unsigned char> host(pel);
	if (vips_hip_memcpy_d2h(host.data(), (const unsigned char *) in->data + (size_t) y * in->stride + (size_t) x * pel, pel))
		return -1;
	// vips_cast to double, getpoint.c:115: every value of every format is a double
	for (int b = 0; b < in->bands; b++)
		switch (in->format) {
		case VIPS_HIP_FORMAT_UCHAR: out[b] = element<unsigned char>(host.data(), b); break;
		case VIPS_HIP_FORMAT_CHAR: out[b] = element<signed char>(host.data(), b); break;
		case VIPS_HIP_FORMAT_USHORT: out[b] = element<unsigned short>(host.data(), b); break;
		case VIPS_HIP_FORMAT_SHORT: out[b] = element<short>(host.data(), b); break;
		case VIPS_HIP_FORMAT_UINT: out[b] = element<unsigned int>(host.data(), b); break;
		case VIPS_HIP_FORMAT_INT: out[b] = element<int>(host.data(), b); break;
		case VIPS_HIP_FORMAT_FLOAT: out[b] = element<float>(host.data(), b); break;
		default: out[b] = element<double>(host.data(), b); break;
		}
	return 0;
}

void vips_hip_find_trim_defaults(VipsHipFindTrim *args)
{
	if (!args)
		return;
	memset(args, 0, sizeof(*args));
	args->threshold = 10.0;
}

double vips_hip_find_trim_background(int interpretation)
{
	switch (interpretation) {
	case VIPS_HIP_INTERPRETATION_GREY16:
	case VIPS_HIP_INTERPRETATION_RGB16:
		return 65535.0;
	case VIPS_HIP_INTERPRETATION_scRGB:
		return 1.0;
	default:
		return 255.0;
	}
}

int vips_hip_find_trim_finish(const unsigned int *columns, int width, const unsigned int *rows, int height, int *left,
	int *top, int *out_width, int *out_height)
{
	if (!columns || !rows || !left || !top || !out_width || !out_height || width < 1 || height < 1) {
		error("find_trim", "bad arguments");
		return -1;
	}
	// vips_profile of a one-row image gives the x of its first non-zero pel or Xsize, vips_avg of that one number is the
	// number; the flipped image gives the distance of the last one from the far end (find_trim.c:145-160)
	double l = width, r = width, t = height, b = height;
	for (int x = 0; x < width; x++)
		if (columns[x]) {
			l = x;
			break;
		}
	for (int x = 0; x < width; x++)
		if (columns[width - 1 - x]) {
			r = x;
			break;
		}
	for (int y = 0; y < height; y++)
		if (rows[y]) {
			t = y;
			break;
		}
	for (int y = 0; y < height; y++)
		if (rows[height - 1 - y]) {
			b = y;
			break;
		}
	// find_trim.c:163-168
	const double w = (width - r) - l, h = (height - b) - t;
	*left = (int) l;
	*top = (int) t;
	*out_width = (int) (w > 0 ? w : 0);
	*out_height = (int) (h > 0 ? h : 0);
	return 0;
}

int vips_hip_find_trim_table(const VipsHipFindTrim *args, int bands, int interpretation, int *fused_out, unsigned char *table)
{
	const char *domain = "find_trim";
	if (!fused_out || bands < 1) {
		error(domain, "bad arguments");
		return -1;
	}
	if (check_args(domain, args))
		return -1;
	VipsHipFindTrim s;
	settle(args, interpretation, &s);
	VipsHipLinear l;
	linear_args(s, &l);
	int out_bands, out_format, single;
	double a_ready[VIPS_HIP_ARITH_MAX_VECTOR], b_ready[VIPS_HIP_ARITH_MAX_VECTOR];
	*fused_out = 0;
	if (bands > VIPS_HIP_ARITH_MAX_VECTOR && s.n_background == 1)
		return 0; // (the single-element loops: any number of bands; the composed route takes it)
	if (vips_hip_linear_plan(&l, bands, VIPS_HIP_FORMAT_UCHAR, &out_bands, &out_format, &single, a_ready, b_ready))
		return -1;
	if (bands > 4 || out_bands != bands || !table)
		return 0;
	// the constant as vips_hip_relational_const takes it on linear's output: int when it is integral AND the image an
	// integer format (relational.c:528-529), which a float image is not
	int const_bands, is_int, c_int[VIPS_HIP_LOGIC_MAX_VECTOR];
	double c_double[VIPS_HIP_LOGIC_MAX_VECTOR];
	if (vips_hip_const_plan("relational_const", &s.threshold, 1, bands, out_format, &const_bands, &is_int, c_int, c_double))
		return -1;
	const bool compare_int = is_int && format_isint(out_format);
	const float a1 = (float) a_ready[0], b1 = (float) b_ready[0];
	for (int b = 0; b < bands; b++)
		for (int v = 0; v < 256; v++) {
			// linear.c:213-235 for a uchar pel and float output: LOOP1 in float, LOOPN in double and rounded by the store
			const float x = (float) (unsigned char) v;
			const float lin = single ? a1 * x + b1 : (float) (a_ready[b] * (double) x + b_ready[b]);
			const float mag = fabsf(lin); // abs.c:107-110
			// RLOOPCI / RLOOPCF, relational.c:472-492
			const bool more = compare_int ? (int) mag > c_int[b] : (double) mag > c_double[b];
			table[b * 256 + v] = more ? 255 : 0;
		}
	*fused_out = 1;
	return 0;
}

int vips_hip_find_trim(VipsHipImage *in, const VipsHipFindTrim *args, int *left, int *top, int *width, int *height)
{
	const char *domain = "find_trim";
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !left || !top || !width || !height) {
		error(domain, "null argument");
		return -1;
	}
	if (check_args(domain, args))
		return -1;
	VipsHipFindTrim s;
	settle(args, in->interpretation, &s);
	// find_trim.c:99-108
	ImageRef flat;
	VipsHipImage *cur = in;
	if (hasalpha(in)) {
		VipsHipFlatten f;
		vips_hip_flatten_defaults(&f);
		f.n_background = s.n_background;
		for (int i = 0; i < s.n_background; i++)
			f.background[i] = s.background[i];
		if (vips_hip_flatten(in, &flat.im, &f))
			return -1;
		cur = flat.im;
	}
	// vips_rank_build's check (rank.c:479-483): the chain's median comes before its linear, so this is said first on
	// either route
	if (!s.line_art && (cur->width < 3 || cur->height < 3)) {
		error("rank", "window too large");
		return -1;
	}
	if (cur->format == VIPS_HIP_FORMAT_UCHAR && cur->bands <= 4 && !getenv("VIPS_HIP_NO_TRIM_FUSED")) {
		unsigned char table[TABLE_BYTES];
		int takes;
		if (vips_hip_find_trim_table(&s, cur->bands, in->interpretation, &takes, table))
			return -1;
		if (takes)
			return fused(cur, s, table, left, top, width, height);
	}
	return composed(cur, s, left, top, width, height);
}

int vips_hip_trim_step(int what)
{
	return trim_tile(what);
}

} // extern "C"
