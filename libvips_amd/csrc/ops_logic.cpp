// vips_relational / vips_relational_const, vips_boolean / vips_boolean_const (arithmetic/relational.c, boolean.c,
// unaryconst.c), vips_ifthenelse (conversion/ifthenelse.c), vips_bandjoin / vips_bandjoin_const, vips_extract_band,
// vips_bandmean and vips_bandbool (conversion/bandjoin.c, extract.c, bandmean.c, bandbool.c, bandary.c) on images in
// HBM: the host side -- each build() restated (the format tables, vips__formatalike / vips__bandalike /
// vips__sizealike over two, three or n images, the constants' c_int / c_double / is_int, the errors with the
// reference's words, the header of the result), the region checks, the C ABI.  The kernels are in logic.hip.
#include "internal.h"

#include <cstring>
#include <vector>

using namespace vh;

static_assert(LOGIC_MAX_VECTOR == VIPS_HIP_LOGIC_MAX_VECTOR, "one length for the constants");
static_assert(RELATIONAL_LAST == VIPS_HIP_RELATIONAL_LAST && BOOLEAN_LAST == VIPS_HIP_BOOLEAN_LAST, "one list of operations");
static_assert(BAND_MAX_SOURCES == VIPS_HIP_BANDJOIN_MAX, "one length for bandjoin's array");

namespace {

// vips_enum_nick of VipsOperationBoolean
const char *const BOOLEAN_NICKS[BOOLEAN_LAST] = { "and", "or", "eor", "lshift", "rshift" };

int check_op(const char *domain, int op, int last)
{
	if (op < 0 || op >= last) {
		error(domain, "bad operation %d", op);
		return -1;
	}
	return 0;
}

// arithmetic_window_pair, and rows that the kernels can index
int check_window_pair(const char *domain, const VipsHipRegion *in, const VipsHipRegion *out)
{
	if (arithmetic_window_pair(domain, in, out))
		return -1;
	if ((long long) out->width * out->bands >= (1LL << 31) || (long long) in->width * in->bands >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	return 0;
}

int check_output(const char *domain, const VipsHipRegion *out, int bands, int format)
{
	if (out->bands != bands || out->format != format) {
		error(domain, "the output must have %d bands of format %d", bands, format);
		return -1;
	}
	return 0;
}

// vips__bandalike_vec (arithmetic.c:210-254) over n images: the most bands of any, the interpretation of the LAST image
// that has them, and the header's interpretation of image 0 once it is matched (shared with ops_nary.cpp)
} // namespace

int vh::bandalike(const char *domain, const int *bands, const int *interpretations, int n, int *out_bands, int *interpretation)
{
	int most = 1, type = interpretations[0];
	for (int i = 0; i < n; i++)
		if (bands[i] >= most) {
			most = bands[i];
			type = interpretations[i];
		}
	for (int i = 0; i < n; i++)
		if (bands[i] != most && bands[i] != 1) {
			error(domain, "not one band or %d bands", most); // vips__bandup, arithmetic.c:184-187
			return -1;
		}
	*out_bands = most;
	*interpretation = bands[0] == most ? interpretations[0] : type;
	return 0;
}

namespace {

struct ConstCall {
	int family, op;
	const double *c;
	int n;
};

const char *const CONST_NICKNAMES[2] = { "relational_const", "boolean_const" };
const char *const BINARY_NICKNAMES[2] = { "relational", "boolean" };

int const_gen(const ConstCall &call, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = CONST_NICKNAMES[call.family];
	if (ensure_init())
		return -1;
	if (check_op(domain, call.op, call.family == LOGIC_RELATIONAL ? RELATIONAL_LAST : BOOLEAN_LAST) || check_window_pair(domain, in, out))
		return -1;
	LogicArgs a;
	memset(&a, 0, sizeof(a));
	int bands, is_int;
	std::vector<int> ci(in->bands > LOGIC_MAX_VECTOR ? in->bands : LOGIC_MAX_VECTOR);
	std::vector<double> cd(ci.size());
	if (vips_hip_const_plan(domain, call.c, call.n, in->bands, in->format, &bands, &is_int, ci.data(), cd.data()))
		return -1;
	if (check_output(domain, out, bands, vips_hip_logic_format(call.family, in->format)))
		return -1;
	a.single = 1;
	for (int i = 1; i < bands; i++)
		if (ci[i] != ci[0] || cd[i] != cd[0])
			a.single = 0;
	if (!a.single && bands > LOGIC_MAX_VECTOR) {
		error(domain, "vectors of more than %d elements are outside the HIP path", LOGIC_MAX_VECTOR);
		return -1;
	}
	for (int i = 0; i < LOGIC_MAX_VECTOR && i < bands; i++) {
		a.c_int[i] = ci[i];
		a.c_double[i] = cd[i];
	}
	// relational.c:528-529; boolean_const uses c_int whatever the constants were
	a.is_int = is_int && !format_iscomplex(in->format) && in->format <= VIPS_HIP_FORMAT_INT;
	pointwise_unary_geom(in, out, &a);
	return logic_run(domain, call.family, call.op, in->format, a);
}

int const_image(int family, VipsHipImage *in, VipsHipImage **out, int op, const double *c, int n)
{
	const char *domain = CONST_NICKNAMES[family];
	if (enter(domain, in, out))
		return -1;
	// boolean.c:476-479; relational.c compares complex numbers, which stay out
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	int bands;
	if (vips_hip_const_plan(domain, c, n, in->bands, in->format, &bands, nullptr, nullptr, nullptr))
		return -1;
	const ConstCall call = { family, op, c, n };
	return whole_image(in, out, bands, vips_hip_logic_format(family, in->format),
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return const_gen(call, ri, ro); });
}

// closure: the family and the operation, which is checked here: behind the device check, before the plan
int binary_plan(const void *closure, const VipsHipImage *left, const VipsHipImage *right, BinaryOperands *b)
{
	const int family = ((const int *) closure)[0], op = ((const int *) closure)[1];
	if (check_op(BINARY_NICKNAMES[family], op, family == LOGIC_RELATIONAL ? RELATIONAL_LAST : BOOLEAN_LAST))
		return -1;
	return vips_hip_logic_plan(family, left->width, left->height, left->bands, left->format, left->interpretation, right->width,
		right->height, right->bands, right->format, right->interpretation, &b->format, &b->out_format, &b->bands, &b->interpretation,
		&b->width, &b->height);
}

int binary_image(int family, VipsHipImage *left, VipsHipImage *right, VipsHipImage **out, int op)
{
	const char *domain = BINARY_NICKNAMES[family];
	if (enter(domain, left, out))
		return -1;
	if (!right) {
		error(domain, "null argument");
		return -1;
	}
	const int call[2] = { family, op };
	BinaryOperands b;
	if (binary_operands(domain, left, right, binary_plan, call, &b))
		return -1;
	LogicArgs a;
	memset(&a, 0, sizeof(a));
	static_cast<PointwiseGeom &>(a) = b.geom;
	a.single = 1;
	if (logic_run(domain, family, op, b.format, a))
		return -1;
	*out = b.out.release();
	return 0;
}

// one source of a band kernel: all of a window
void source_of(const VipsHipRegion *in, BandSource *s)
{
	memset(s, 0, sizeof(*s));
	s->in = (const unsigned char *) in->data;
	s->stride = (long long) in->stride;
	s->pel_elems = in->bands;
	s->end = in->bands;
	s->width = in->width;
	s->height = in->height;
}

void band_output(const VipsHipRegion *out, BandArgs *a)
{
	memset(a, 0, sizeof(*a));
	a->out = (unsigned char *) out->data;
	a->out_stride = (long long) out->stride;
	a->elems = out->width * out->bands;
	a->height = out->height;
	a->out_bands = out->bands;
}

int check_bandbool(int op)
{
	const char *domain = "bandbool";
	if (check_op(domain, op, BOOLEAN_LAST))
		return -1;
	// bandbool.c:72-80
	if (op == BOOLEAN_LSHIFT || op == BOOLEAN_RSHIFT) {
		error(domain, "operator %s not supported across image bands", BOOLEAN_NICKS[op]);
		return -1;
	}
	return 0;
}

// extract.c:402-406
int check_extract(int band, int n, int bands)
{
	if (band < 0 || n < 1 || (unsigned long long) band + (unsigned long long) n > (unsigned long long) bands) {
		error("extract_band", "bad extract band");
		return -1;
	}
	return 0;
}

} // namespace

extern "C" {

int vips_hip_logic_format(int boolean, int format)
{
	enum { UC, C, US, S, UI, I };
	static const int tables[2][10] = {
		/* relational.c:214-217 */ { UC, UC, UC, UC, UC, UC, UC, UC, UC, UC },
		/* boolean.c:253-256, bandbool.c:213-216 */ { UC, C, US, S, UI, I, I, I, I, I },
	};
	if (format < 0 || format > VIPS_HIP_FORMAT_DPCOMPLEX)
		return -1;
	return tables[boolean ? 1 : 0][format];
}

int vips_hip_const_plan(const char *nickname, const double *c, int n, int bands, int format, int *out_bands, int *is_int,
	int *c_int, double *c_double)
{
	const char *domain = nickname ? nickname : "unary_const";
	if (!c || !out_bands || bands < 1) {
		error(domain, "bad arguments");
		return -1;
	}
	if (arithmetic_noncomplex(domain, format))
		return -1;
	if (n < 1) {
		error(domain, "vector must have at least 1 element");
		return -1;
	}
	// vips_check_vector, iofuncs/error.c:1118-1140
	if (!(n == bands || n == 1 || bands == 1)) {
		error(domain, "vector must have 1 or %d elements", bands);
		return -1;
	}
	// unaryconst.c:66-71: a one-band image against n elements is banded up
	const int most = n > bands ? n : bands;
	*out_bands = most;
	// unaryconst.c:100-113
	int all_int = 1;
	for (int i = 0; i < most; i++) {
		const double d = c[i < n - 1 ? i : n - 1];
		// c_int[i] = c_double[i]: in range the truncation toward zero; out of range (and NaN) the reference's processor
		// gives INT_MIN ("integer indefinite"), written out here so that no compiler's choice enters
		const int v = d > -2147483649.0 && d < 2147483648.0 ? (int) d : (-2147483647 - 1);
		if (c_double)
			c_double[i] = d;
		if (c_int)
			c_int[i] = v;
		if (v != d)
			all_int = 0;
	}
	if (is_int)
		*is_int = all_int;
	return 0;
}

int vips_hip_logic_plan(int boolean, int left_width, int left_height, int left_bands, int left_format, int left_interpretation,
	int right_width, int right_height, int right_bands, int right_format, int right_interpretation, int *format,
	int *out_format, int *bands, int *interpretation, int *width, int *height)
{
	const char *domain = BINARY_NICKNAMES[boolean ? 1 : 0];
	if (!format || !out_format || !bands || !interpretation || !width || !height) {
		error(domain, "null argument");
		return -1;
	}
	if (left_width < 1 || left_height < 1 || left_bands < 1 || right_width < 1 || right_height < 1 || right_bands < 1) {
		error(domain, "bad image size");
		return -1;
	}
	// boolean.c:76-81; relational.c compares complex numbers, which stay out
	if (arithmetic_noncomplex(domain, left_format) || arithmetic_noncomplex(domain, right_format))
		return -1;
	*format = format_common(left_format, right_format);
	*out_format = vips_hip_logic_format(boolean, *format);
	const int b[2] = { left_bands, right_bands }, t[2] = { left_interpretation, right_interpretation };
	if (bandalike(domain, b, t, 2, bands, interpretation))
		return -1;
	*width = left_width > right_width ? left_width : right_width;
	*height = left_height > right_height ? left_height : right_height;
	return 0;
}

int vips_hip_ifthenelse_plan(int cond_width, int cond_height, int cond_bands, int cond_format, int cond_interpretation,
	int then_width, int then_height, int then_bands, int then_format, int then_interpretation, int else_width, int else_height,
	int else_bands, int else_format, int else_interpretation, int *format, int *bands, int *interpretation, int *width,
	int *height)
{
	const char *domain = "ifthenelse";
	if (!format || !bands || !interpretation || !width || !height) {
		error(domain, "null argument");
		return -1;
	}
	if (cond_width < 1 || cond_height < 1 || cond_bands < 1 || then_width < 1 || then_height < 1 || then_bands < 1 ||
		else_width < 1 || else_height < 1 || else_bands < 1) {
		error(domain, "bad image size");
		return -1;
	}
	if (arithmetic_noncomplex(domain, cond_format) || arithmetic_noncomplex(domain, then_format) || arithmetic_noncomplex(domain, else_format))
		return -1;
	// ifthenelse.c:479-486: then, else, condition -- the output's header is the then image's
	const int b[3] = { then_bands, else_bands, cond_bands };
	const int t[3] = { then_interpretation, else_interpretation, cond_interpretation };
	if (bandalike(domain, b, t, 3, bands, interpretation))
		return -1;
	*format = format_common(then_format, else_format); // ifthenelse.c:503
	*width = then_width > else_width ? then_width : else_width;
	*width = cond_width > *width ? cond_width : *width;
	*height = then_height > else_height ? then_height : else_height;
	*height = cond_height > *height ? cond_height : *height;
	return 0;
}

int vips_hip_bandjoin_plan(int n, const int *widths, const int *heights, const int *bands, const int *formats,
	int interpretation0, int *format, int *out_bands, int *interpretation, int *width, int *height)
{
	const char *domain = "bandjoin";
	if (!widths || !heights || !bands || !formats || !format || !out_bands || !interpretation || !width || !height) {
		error(domain, "null argument");
		return -1;
	}
	if (n < 1) {
		error(domain, "no input images"); // bandary.c:204-208
		return -1;
	}
	if (n > BAND_MAX_SOURCES) {
		error(domain, "arrays of more than %d images are outside the HIP path", BAND_MAX_SOURCES);
		return -1;
	}
	long long sum = 0;
	*width = *height = 0;
	*format = formats[0];
	for (int i = 0; i < n; i++) {
		if (widths[i] < 1 || heights[i] < 1 || bands[i] < 1) {
			error(domain, "bad image size");
			return -1;
		}
		if (arithmetic_noncomplex(domain, formats[i]))
			return -1;
		// vips__formatalike_vec, vips__sizealike_vec (bandary.c:217-219); bandjoin.c:147-151
		*format = i ? format_common(*format, formats[i]) : formats[0];
		*width = widths[i] > *width ? widths[i] : *width;
		*height = heights[i] > *height ? heights[i] : *height;
		sum += bands[i];
	}
	if (sum * *width >= (1LL << 31) / 8) {
		error(domain, "image rows too long");
		return -1;
	}
	*out_bands = (int) sum;
	*interpretation = interpretation0; // bandary.c:222: the header is ready[0]'s
	return 0;
}

int vips_hip_relational_const_gen(int relational, const double *c, int n, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const ConstCall call = { LOGIC_RELATIONAL, relational, c, n };
	return const_gen(call, in, out);
}

int vips_hip_boolean_const_gen(int boolean, const double *c, int n, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const ConstCall call = { LOGIC_BOOLEAN, boolean, c, n };
	return const_gen(call, in, out);
}

int vips_hip_relational_const(VipsHipImage *in, VipsHipImage **out, int relational, const double *c, int n)
{
	return const_image(LOGIC_RELATIONAL, in, out, relational, c, n);
}

int vips_hip_boolean_const(VipsHipImage *in, VipsHipImage **out, int boolean, const double *c, int n)
{
	return const_image(LOGIC_BOOLEAN, in, out, boolean, c, n);
}

int vips_hip_relational(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out, int relational)
{
	return binary_image(LOGIC_RELATIONAL, left, right, out, relational);
}

int vips_hip_boolean(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out, int boolean)
{
	return binary_image(LOGIC_BOOLEAN, left, right, out, boolean);
}

int vips_hip_ifthenelse(VipsHipImage *cond, VipsHipImage *in1, VipsHipImage *in2, VipsHipImage **out, int blend)
{
	const char *domain = "ifthenelse";
	if (enter(domain, cond, out))
		return -1;
	if (!in1 || !in2) {
		error(domain, "null argument");
		return -1;
	}
	if (in1->device != cond->device || in2->device != cond->device) {
		error(domain, "the images are on different devices");
		return -1;
	}
	int format, bands, interpretation, width, height;
	if (vips_hip_ifthenelse_plan(cond->width, cond->height, cond->bands, cond->format, cond->interpretation, in1->width,
			in1->height, in1->bands, in1->format, in1->interpretation, in2->width, in2->height, in2->bands, in2->format,
			in2->interpretation, &format, &bands, &interpretation, &width, &height))
		return -1;
	// ifthenelse.c:494-504: the condition through vips_cast to uchar (it clips), then and else to their common format
	ImageRef cast[3];
	VipsHipImage *im[3] = { cond, in1, in2 };
	const int want[3] = { VIPS_HIP_FORMAT_UCHAR, format, format };
	for (int i = 0; i < 3; i++)
		if (im[i]->format != want[i]) {
			if (vips_hip_cast(im[i], &cast[i].im, want[i]))
				return -1;
			im[i] = cast[i].im;
		}
	if ((long long) width * bands >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	ImageRef o(vips_hip_image_new(width, height, bands, format, interpretation));
	if (!o.im)
		return -1;
	SelectArgs a;
	memset(&a, 0, sizeof(a));
	a.cond = (const unsigned char *) im[0]->data;
	a.in = (const unsigned char *) im[1]->data;
	a.in2 = (const unsigned char *) im[2]->data;
	a.out = (unsigned char *) o.im->data;
	a.cond_stride = (long long) im[0]->stride;
	a.in_stride = (long long) im[1]->stride;
	a.in2_stride = (long long) im[2]->stride;
	a.out_stride = (long long) o.im->stride;
	a.elems = width * bands;
	a.height = height;
	a.bands = bands;
	a.wc = im[0]->width, a.hc = im[0]->height, a.bc = im[0]->bands;
	a.w1 = im[1]->width, a.h1 = im[1]->height, a.b1 = im[1]->bands;
	a.w2 = im[2]->width, a.h2 = im[2]->height, a.b2 = im[2]->bands;
	if (select_run(domain, format, blend != 0, a))
		return -1;
	*out = o.release();
	return 0;
}

int vips_hip_bandjoin(VipsHipImage **in, int n, VipsHipImage **out)
{
	const char *domain = "bandjoin";
	if (!in || !out || n < 1 || !in[0]) {
		error(domain, n < 1 && in && out ? "no input images" : "null argument");
		return -1;
	}
	if (bind_to(in[0]))
		return -1;
	if (n > BAND_MAX_SOURCES) {
		error(domain, "arrays of more than %d images are outside the HIP path", BAND_MAX_SOURCES);
		return -1;
	}
	int widths[BAND_MAX_SOURCES], heights[BAND_MAX_SOURCES], bands[BAND_MAX_SOURCES], formats[BAND_MAX_SOURCES];
	for (int i = 0; i < n; i++) {
		if (!in[i]) {
			error(domain, "null argument");
			return -1;
		}
		if (in[i]->device != in[0]->device) {
			error(domain, "the images are on different devices");
			return -1;
		}
		widths[i] = in[i]->width;
		heights[i] = in[i]->height;
		bands[i] = in[i]->bands;
		formats[i] = in[i]->format;
	}
	int format, out_bands, interpretation, width, height;
	if (vips_hip_bandjoin_plan(n, widths, heights, bands, formats, in[0]->interpretation, &format, &out_bands, &interpretation,
			&width, &height))
		return -1;
	// bandjoin.c:143-144: one image is a copy
	if (n == 1)
		return vips_hip_cast(in[0], out, in[0]->format);
	ImageRef cast[BAND_MAX_SOURCES];
	ImageRef o(vips_hip_image_new(width, height, out_bands, format, interpretation));
	if (!o.im)
		return -1;
	VipsHipRegion ro;
	vips_hip_image_region(o.im, &ro);
	BandArgs a;
	band_output(&ro, &a);
	a.n = n;
	int at = 0;
	for (int i = 0; i < n; i++) {
		VipsHipImage *im = in[i];
		if (im->format != format) {
			if (vips_hip_cast(im, &cast[i].im, format))
				return -1;
			im = cast[i].im;
		}
		VipsHipRegion ri;
		vips_hip_image_region(im, &ri);
		source_of(&ri, &a.src[i]);
		a.src[i].begin = at;
		a.src[i].end = at += im->bands;
	}
	if (band_run(domain, BAND_JOIN, format, a))
		return -1;
	*out = o.release();
	return 0;
}

int vips_hip_bandjoin_const_gen(const double *c, int n, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = "bandjoin_const";
	if (ensure_init())
		return -1;
	if (check_window_pair(domain, in, out))
		return -1;
	if (!c || n < 1 || n > BAND_MAX_SOURCES - 1) {
		error(domain, "1 to %d constants", BAND_MAX_SOURCES - 1);
		return -1;
	}
	if (check_output(domain, out, in->bands + n, in->format))
		return -1;
	// bandjoin.c:380-385: vips__vector_to_pels -- the constants through vips_linear and vips_cast
	const int es = format_sizeof(in->format);
	std::vector<unsigned char> ink((size_t) n * es);
	if (vips_hip_vector_to_ink(c, n, n, in->format, ink.data()))
		return -1;
	BandArgs a;
	band_output(out, &a);
	a.n = n + 1;
	source_of(in, &a.src[0]);
	for (int i = 0; i < n; i++) {
		BandSource *s = &a.src[i + 1];
		memset(s, 0, sizeof(*s));
		memcpy(&s->value, ink.data() + (size_t) i * es, es); // (little-endian: the element is the value's low bytes)
		s->begin = in->bands + i;
		s->end = s->begin + 1;
	}
	return band_run(domain, BAND_JOIN, in->format, a);
}

int vips_hip_bandjoin_const(VipsHipImage *in, VipsHipImage **out, const double *c, int n)
{
	const char *domain = "bandjoin_const";
	if (enter(domain, in, out))
		return -1;
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	// bandjoin.c:360-362: no constants is a copy
	if (n == 0)
		return vips_hip_cast(in, out, in->format);
	if (!c || n < 1 || n > BAND_MAX_SOURCES - 1) {
		error(domain, "1 to %d constants", BAND_MAX_SOURCES - 1);
		return -1;
	}
	return whole_image(in, out, in->bands + n, in->format,
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_bandjoin_const_gen(c, n, ri, ro); });
}

int vips_hip_extract_band_gen(int band, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = "extract_band";
	if (ensure_init())
		return -1;
	if (check_window_pair(domain, in, out))
		return -1;
	if (check_extract(band, out->bands, in->bands) || check_output(domain, out, out->bands, in->format))
		return -1;
	BandArgs a;
	band_output(out, &a);
	a.n = 1;
	source_of(in, &a.src[0]);
	a.src[0].first = band;
	a.src[0].end = out->bands;
	return band_run(domain, BAND_JOIN, in->format, a);
}

int vips_hip_extract_band(VipsHipImage *in, VipsHipImage **out, int band, int n)
{
	const char *domain = "extract_band";
	if (enter(domain, in, out))
		return -1;
	if (arithmetic_noncomplex(domain, in->format) || check_extract(band, n, in->bands))
		return -1;
	// extract.c:408-410
	if (band == 0 && n == in->bands)
		return vips_hip_cast(in, out, in->format);
	return whole_image(in, out, n, in->format,
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_extract_band_gen(band, ri, ro); });
}

int vips_hip_bandmean_gen(const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = "bandmean";
	if (ensure_init())
		return -1;
	if (check_window_pair(domain, in, out) || check_output(domain, out, 1, in->format))
		return -1;
	BandArgs a;
	band_output(out, &a);
	a.n = 1;
	source_of(in, &a.src[0]);
	return band_run(domain, BAND_MEAN, in->format, a);
}

int vips_hip_bandmean(VipsHipImage *in, VipsHipImage **out)
{
	const char *domain = "bandmean";
	if (enter(domain, in, out))
		return -1;
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	// bandmean.c:162-164
	if (in->bands == 1)
		return vips_hip_cast(in, out, in->format);
	return whole_image(in, out, 1, in->format, vips_hip_bandmean_gen);
}

int vips_hip_bandbool_gen(int boolean, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = "bandbool";
	if (ensure_init())
		return -1;
	if (check_bandbool(boolean) || check_window_pair(domain, in, out) ||
		check_output(domain, out, 1, vips_hip_logic_format(1, in->format)))
		return -1;
	BandArgs a;
	band_output(out, &a);
	a.n = 1;
	source_of(in, &a.src[0]);
	return band_run(domain, BAND_AND + boolean, in->format, a);
}

int vips_hip_bandbool(VipsHipImage *in, VipsHipImage **out, int boolean)
{
	const char *domain = "bandbool";
	if (check_bandbool(boolean)) // bandbool.c:72-80: before the image is looked at
		return -1;
	if (enter(domain, in, out))
		return -1;
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	// bandbool.c:89-90: one band is a copy (of the image as it is: a float image stays float)
	if (in->bands == 1)
		return vips_hip_cast(in, out, in->format);
	return whole_image(in, out, 1, vips_hip_logic_format(1, in->format),
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_bandbool_gen(boolean, ri, ro); });
}

int vips_hip_logic_step(int what)
{
	return logic_tile(what);
}

} // extern "C"
