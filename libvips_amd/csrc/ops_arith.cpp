// vips_linear, vips_invert, vips_abs, vips_add, vips_subtract, vips_multiply, vips_divide, vips_round, vips_sign,
// vips_clamp, vips_minpair, vips_maxpair, vips_remainder, vips_remainder_const, vips_stats, vips_avg, vips_deviate,
// vips_min and vips_max (arithmetic/*.c) on images in HBM: the host side -- each build() restated (the
// format tables, vips_linear's vectors and its single-element rule, vips__formatalike / vips__bandalike /
// vips__sizealike for two images, the errors with the reference's words), the merge of the statistics' partials and
// the reference's avg / sd / row-0 expressions, the region checks, the C ABI.  The kernels are in arith.hip.
#include "internal.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace vh;

static_assert(ARITH_MAX_VECTOR == VIPS_HIP_ARITH_MAX_VECTOR, "one length for vips_linear's vectors");
static_assert(ARITH_LAST == VIPS_HIP_ARITH_LAST, "one list of operations");

namespace {

const char *const NICKNAMES[ARITH_LAST] = { "linear", "invert", "abs", "add", "subtract", "multiply", "divide", "round", "sign",
	"clamp", "minpair", "maxpair", "remainder", "remainder_const" };

} // namespace

// arithmetic.c:76-109
int vh::format_common(int a, int b)
{
	enum { UC, C, US, S, UI, I };
	static const int largest[6][6] = {
		/* UC */ { UC, S, US, S, UI, I },
		/* C */ { S, C, I, S, I, I },
		/* US */ { US, I, US, I, UI, I },
		/* S */ { S, S, I, S, I, I },
		/* UI */ { UI, I, UI, I, UI, I },
		/* I */ { I, I, I, I, I, I },
	};
	if (a == VIPS_HIP_FORMAT_DOUBLE || b == VIPS_HIP_FORMAT_DOUBLE)
		return VIPS_HIP_FORMAT_DOUBLE;
	if (a == VIPS_HIP_FORMAT_FLOAT || b == VIPS_HIP_FORMAT_FLOAT)
		return VIPS_HIP_FORMAT_FLOAT;
	return largest[a][b];
}

int vh::arithmetic_window_pair(const char *domain, const VipsHipRegion *in, const VipsHipRegion *out)
{
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (arithmetic_noncomplex(domain, in->format) || arithmetic_noncomplex(domain, out->format))
		return -1;
	if (in->width != out->width || in->height != out->height) {
		error(domain, "input and output regions must have the same size");
		return -1;
	}
	if (in->data == out->data) {
		error(domain, "cannot work in place");
		return -1;
	}
	return 0;
}

void vh::pointwise_unary_geom(const VipsHipRegion *in, const VipsHipRegion *out, PointwiseGeom *g)
{
	memset(g, 0, sizeof(*g));
	g->in = (const unsigned char *) in->data;
	g->out = (unsigned char *) out->data;
	g->in_stride = (long long) in->stride;
	g->out_stride = (long long) out->stride;
	g->elems = out->width * out->bands;
	g->height = out->height;
	g->bands = out->bands;
	g->w1 = in->width;
	g->h1 = in->height;
	g->b1 = in->bands;
}

void vh::pointwise_binary_geom(const VipsHipImage *left, const VipsHipImage *right, const VipsHipImage *out, PointwiseGeom *g)
{
	memset(g, 0, sizeof(*g));
	g->in = (const unsigned char *) left->data;
	g->in2 = (const unsigned char *) right->data;
	g->out = (unsigned char *) out->data;
	g->in_stride = (long long) left->stride;
	g->in2_stride = (long long) right->stride;
	g->out_stride = (long long) out->stride;
	g->elems = out->width * out->bands;
	g->height = out->height;
	g->bands = out->bands;
	g->w1 = left->width;
	g->h1 = left->height;
	g->b1 = left->bands;
	g->w2 = right->width;
	g->h2 = right->height;
	g->b2 = right->bands;
}

int vh::binary_operands(const char *domain, VipsHipImage *left, VipsHipImage *right, BinaryPlanFn plan, const void *closure, BinaryOperands *b)
{
	if (right->device != left->device) {
		error(domain, "the images are on different devices");
		return -1;
	}
	if (plan(closure, left, right, b))
		return -1;
	// vips__formatalike (arithmetic.c:111-137): vips_cast of what is not in the common format
	VipsHipImage *im[2] = { left, right };
	for (int i = 0; i < 2; i++)
		if (im[i]->format != b->format) {
			if (vips_hip_cast(im[i], &b->cast[i].im, b->format))
				return -1;
			im[i] = b->cast[i].im;
		}
	if ((long long) b->width * b->bands >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	b->out.im = vips_hip_image_new(b->width, b->height, b->bands, b->out_format, b->interpretation);
	if (!b->out.im)
		return -1;
	pointwise_binary_geom(im[0], im[1], b->out.im, &b->geom);
	return 0;
}

namespace {

// the arguments of a call without vectors
void arith_args(const PointwiseGeom &g, ArithArgs *a)
{
	memset(a, 0, sizeof(*a));
	*static_cast<PointwiseGeom *>(a) = g;
	a->single = 1;
}

void unary_args(const VipsHipRegion *in, const VipsHipRegion *out, ArithArgs *a)
{
	PointwiseGeom g;
	pointwise_unary_geom(in, out, &g);
	arith_args(g, a);
}

// invert and abs: the same bands and format on both sides
int same_gen(int op, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = NICKNAMES[op];
	if (ensure_init())
		return -1;
	if (arithmetic_window_pair(domain, in, out))
		return -1;
	if (in->bands != out->bands || in->format != out->format) {
		error(domain, "input and output must have the same bands and format");
		return -1;
	}
	if ((long long) out->width * out->bands >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	ArithArgs a;
	unary_args(in, out, &a);
	return arith_run(domain, op, in->format, out->format, a);
}

int same_image(int op, VipsHipImage *in, VipsHipImage **out)
{
	const char *domain = NICKNAMES[op];
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	// abs.c:88-90: vips_unary_copy, a pointer copy
	if (op == ARITH_ABS && (in->format == VIPS_HIP_FORMAT_UCHAR || in->format == VIPS_HIP_FORMAT_USHORT || in->format == VIPS_HIP_FORMAT_UINT))
		return vips_hip_cast(in, out, in->format);
	ImageRef o(vips_hip_image_new(in->width, in->height, in->bands, in->format, in->interpretation));
	if (!o.im)
		return -1;
	VipsHipRegion ri, ro;
	vips_hip_image_region(in, &ri);
	vips_hip_image_region(o.im, &ro);
	if (same_gen(op, &ri, &ro))
		return -1;
	*out = o.release();
	return 0;
}

// round, sign, clamp and remainder_const on a pair of windows: `a` holds the operation's own arguments, the output has
// `bands` bands of the format the operation's table gives for the input's
int unary2_gen(int op, const VipsHipRegion *in, const VipsHipRegion *out, int bands, ArithArgs a)
{
	const char *domain = NICKNAMES[op];
	const int format = vips_hip_arith_format(op, in->format);
	if (out->bands != bands || out->format != format) {
		error(domain, "the output must have %d bands of format %d", bands, format);
		return -1;
	}
	if ((long long) out->width * out->bands >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	PointwiseGeom g;
	pointwise_unary_geom(in, out, &g);
	static_cast<PointwiseGeom &>(a) = g;
	return arith_run(domain, op, in->format, out->format, a);
}

// ... how each of them starts
int unary2_enter(int op, const VipsHipRegion *in, const VipsHipRegion *out, ArithArgs *a)
{
	if (ensure_init())
		return -1;
	if (arithmetic_window_pair(NICKNAMES[op], in, out))
		return -1;
	memset(a, 0, sizeof(*a));
	a->single = 1;
	return 0;
}

int check_round(int round)
{
	if (round < 0 || round >= ROUND_LAST) {
		error("round", "bad operation %d", round);
		return -1;
	}
	return 0;
}

int binary_plan(const void *closure, const VipsHipImage *left, const VipsHipImage *right, BinaryOperands *b)
{
	return vips_hip_binary_plan(*(const int *) closure, left->width, left->height, left->bands, left->format, left->interpretation,
		right->width, right->height, right->bands, right->format, right->interpretation, &b->format, &b->out_format, &b->bands,
		&b->interpretation, &b->width, &b->height);
}

int binary_image(int op, VipsHipImage *left, VipsHipImage *right, VipsHipImage **out)
{
	const char *domain = NICKNAMES[op];
	if (left && bind_to(left))
		return -1;
	if (!left || !right || !out) {
		error(domain, "null argument");
		return -1;
	}
	BinaryOperands b;
	if (binary_operands(domain, left, right, binary_plan, &op, &b))
		return -1;
	ArithArgs a;
	arith_args(b.geom, &a);
	if (arith_run(domain, op, b.format, b.out_format, a))
		return -1;
	*out = b.out.release();
	return 0;
}

enum { COL_MIN = 0, COL_MAX, COL_SUM, COL_SUM2, COL_AVG, COL_SD, COL_XMIN, COL_YMIN, COL_XMAX, COL_YMAX, COL_LAST };

template <typename T>
T from_bits(unsigned int bits)
{
	T v;
	memcpy(&v, &bits, sizeof(v));
	return v;
}

// a partial's extreme as the double the reference's matrix holds
double value_of(int format, unsigned int bits)
{
	if (format == VIPS_HIP_FORMAT_FLOAT)
		return (double) from_bits<float>(bits);
	return format == VIPS_HIP_FORMAT_UINT ? (double) bits : (double) from_bits<int>(bits);
}

// the slab's partials of one band, blocks in index order, to row b + 1 of the matrix
void merge_band(const StatsPartial *slab, int blocks, int bands, int b, int format, int width, double *row)
{
	const bool is_float = format == VIPS_HIP_FORMAT_FLOAT;
	long long isum = 0;
	unsigned long long isum2 = 0;
	double fsum = 0.0, fsum2 = 0.0;
	double mn = 0.0, mx = 0.0;
	unsigned int imn = STATS_NONE, imx = STATS_NONE;
	for (int k = 0; k < blocks; k++) {
		const StatsPartial &p = slab[(size_t) k * bands + b];
		if (is_float) {
			double s, s2;
			memcpy(&s, &p.sum, sizeof(s));
			memcpy(&s2, &p.sum2, sizeof(s2));
			fsum += s;
			fsum2 += s2;
		}
		else {
			isum += (long long) p.sum;
			isum2 += p.sum2;
		}
		if (p.imn != STATS_NONE) {
			const double v = value_of(format, p.mn);
			if (imn == STATS_NONE || v < mn || (v == mn && p.imn < imn)) {
				mn = v;
				imn = p.imn;
			}
		}
		if (p.imx != STATS_NONE) {
			const double v = value_of(format, p.mx);
			if (imx == STATS_NONE || v > mx || (v == mx && p.imx < imx)) {
				mx = v;
				imx = p.imx;
			}
		}
	}
	// a band of nothing but NaN: the reference's extremes are the NaN it started from
	row[COL_MIN] = imn == STATS_NONE ? NAN : mn;
	row[COL_MAX] = imx == STATS_NONE ? NAN : mx;
	// the exact integer sums, rounded once
	row[COL_SUM] = is_float ? fsum : (double) isum;
	row[COL_SUM2] = is_float ? fsum2 : (double) isum2;
	row[COL_XMIN] = imn == STATS_NONE ? 0 : (double) (imn % (unsigned int) width);
	row[COL_YMIN] = imn == STATS_NONE ? 0 : (double) (imn / (unsigned int) width);
	row[COL_XMAX] = imx == STATS_NONE ? 0 : (double) (imx % (unsigned int) width);
	row[COL_YMAX] = imx == STATS_NONE ? 0 : (double) (imx / (unsigned int) width);
}

// extremes: the call wants only the extremes and their places (vips_min, vips_max), which uint and int images have too
int stats_matrix(const char *domain, VipsHipImage *in, std::vector<double> *matrix, bool extremes = false)
{
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in) {
		error(domain, "null argument");
		return -1;
	}
	if (arithmetic_noncomplex(domain, in->format)) // stats.c:116, deviate.c:100
		return -1;
	switch (in->format) {
	case VIPS_HIP_FORMAT_UCHAR:
	case VIPS_HIP_FORMAT_CHAR:
	case VIPS_HIP_FORMAT_USHORT:
	case VIPS_HIP_FORMAT_SHORT:
	case VIPS_HIP_FORMAT_FLOAT:
		break;
	case VIPS_HIP_FORMAT_UINT:
	case VIPS_HIP_FORMAT_INT:
		if (extremes)
			break;
		error(domain, "uint, int and double images are outside the HIP path (uchar, char, ushort, short and float only)");
		return -1;
	default:
		if (extremes) {
			error(domain, "double images are outside the HIP path (uchar, char, ushort, short, uint, int and float only)");
			return -1;
		}
		error(domain, "uint, int and double images are outside the HIP path (uchar, char, ushort, short and float only)");
		return -1;
	}
	if (in->width < 1 || in->height < 1 || in->bands < 1) {
		error(domain, "bad image size");
		return -1;
	}
	const int blocks = stats_blocks(in);
	const size_t entries = (size_t) blocks * in->bands;
	DeviceBlock slab(entries * sizeof(StatsPartial));
	if (!slab.p)
		return -1;
	std::vector<StatsPartial> host(entries);
	if (stats_run(domain, in, (StatsPartial *) slab.p) || vips_hip_memcpy_d2h(host.data(), slab.p, entries * sizeof(StatsPartial)))
		return -1;
	matrix->assign((size_t) (in->bands + 1) * COL_LAST, 0.0);
	for (int b = 0; b < in->bands; b++)
		merge_band(host.data(), blocks, in->bands, b, in->format, in->width, matrix->data() + (size_t) (b + 1) * COL_LAST);
	return vips_hip_stats_finish(matrix->data(), in->bands, (long long) in->width * in->height);
}

} // namespace

extern "C" {

void vips_hip_linear_defaults(VipsHipLinear *args)
{
	if (!args)
		return;
	memset(args, 0, sizeof(*args));
	args->n_a = 1;
	args->a[0] = 1.0;
	args->n_b = 1;
}

int vips_hip_arith_format(int op, int format)
{
	enum { UC, C, US, S, UI, I, F, X, D, DX };
	static const int tables[ARITH_LAST][10] = {
		/* linear.c:425-428 */ { F, F, F, F, F, F, F, X, D, DX },
		/* invert.c:166-169 */ { UC, C, US, S, UI, I, F, X, D, DX },
		/* abs.c:188-191 */ { UC, C, US, S, UI, I, F, F, D, D },
		/* add.c:180-183 */ { US, S, UI, I, UI, I, F, X, D, DX },
		/* subtract.c:176-179 */ { S, S, I, I, I, I, F, X, D, DX },
		/* multiply.c:197-200 */ { US, S, UI, I, UI, I, F, X, D, DX },
		/* divide.c:199-202 */ { F, F, F, F, F, F, F, X, D, DX },
		/* round.c:157-160 */ { UC, C, US, S, UI, I, F, X, D, DX },
		/* sign.c:162-165 */ { C, C, C, C, C, C, C, X, C, DX },
		/* clamp.c:139-142 */ { UC, C, US, S, UI, I, F, X, D, DX },
		/* minpair.c:139-142 */ { UC, C, US, S, UI, I, F, X, D, DX },
		/* maxpair.c:139-142 */ { UC, C, US, S, UI, I, F, X, D, DX },
		/* remainder.c:175-178 */ { UC, C, US, S, UI, I, F, X, D, DX },
		/* ... and remainder_const */ { UC, C, US, S, UI, I, F, X, D, DX },
	};
	if (op < 0 || op >= ARITH_LAST || format < 0 || format > VIPS_HIP_FORMAT_DPCOMPLEX || format_iscomplex(format))
		return -1;
	return tables[op][format];
}

int vips_hip_linear_plan(const VipsHipLinear *args, int bands, int format, int *out_bands, int *out_format, int *single,
	double *a_ready, double *b_ready)
{
	const char *domain = "linear";
	VipsHipLinear defaults;
	if (!args) {
		vips_hip_linear_defaults(&defaults);
		args = &defaults;
	}
	if (!out_bands || !out_format || !single || bands < 1) {
		error(domain, "bad arguments");
		return -1;
	}
	if (arithmetic_noncomplex(domain, format))
		return -1;
	if (args->n_a < 1 || args->n_a > VIPS_HIP_ARITH_MAX_VECTOR || args->n_b < 1 || args->n_b > VIPS_HIP_ARITH_MAX_VECTOR) {
		error(domain, "vectors of 1 to %d elements", VIPS_HIP_ARITH_MAX_VECTOR);
		return -1;
	}
	// linear.c:131-145: a one-band image against n elements is banded up
	int n = args->n_a > args->n_b ? args->n_a : args->n_b;
	n = bands > n ? bands : n;
	// vips_check_vector, iofuncs/error.c:1118-1140
	for (const int len : { args->n_a, args->n_b })
		if (!(len == bands || len == 1 || bands == 1)) {
			error(domain, "vector must have 1 or %d elements", bands);
			return -1;
		}
	// linear.c:155-179: a vector whose elements are all equal counts as one element
	int a_n = 1, b_n = 1;
	for (int i = 1; i < args->n_a; i++)
		if (args->a[i] != args->a[0]) {
			a_n = args->n_a;
			break;
		}
	for (int i = 1; i < args->n_b; i++)
		if (args->b[i] != args->b[0]) {
			b_n = args->n_b;
			break;
		}
	*single = a_n == 1 && b_n == 1;
	if (!*single && n > VIPS_HIP_ARITH_MAX_VECTOR) {
		error(domain, "vectors of more than %d elements are outside the HIP path", VIPS_HIP_ARITH_MAX_VECTOR);
		return -1;
	}
	// linear.c:181-200
	for (int i = 0; i < VIPS_HIP_ARITH_MAX_VECTOR; i++) {
		const int ia = i < a_n - 1 ? i : a_n - 1, ib = i < b_n - 1 ? i : b_n - 1;
		if (a_ready)
			a_ready[i] = i < n ? args->a[ia] : 0.0;
		if (b_ready)
			b_ready[i] = i < n ? args->b[ib] : 0.0;
	}
	*out_bands = n;
	*out_format = args->uchar ? VIPS_HIP_FORMAT_UCHAR : vips_hip_arith_format(ARITH_LINEAR, format); // linear.c:202-203
	return 0;
}

int vips_hip_binary_plan(int op, int left_width, int left_height, int left_bands, int left_format, int left_interpretation,
	int right_width, int right_height, int right_bands, int right_format, int right_interpretation, int *format,
	int *out_format, int *bands, int *interpretation, int *width, int *height)
{
	if (!arith_binary(op)) {
		error("arithmetic", "not a binary operation: %d", op);
		return -1;
	}
	const char *domain = NICKNAMES[op];
	if (!format || !out_format || !bands || !interpretation || !width || !height) {
		error(domain, "null argument");
		return -1;
	}
	if (left_width < 1 || left_height < 1 || left_bands < 1 || right_width < 1 || right_height < 1 || right_bands < 1) {
		error(domain, "bad image size");
		return -1;
	}
	if (arithmetic_noncomplex(domain, left_format) || arithmetic_noncomplex(domain, right_format))
		return -1;
	*format = format_common(left_format, right_format);
	*out_format = vips_hip_arith_format(op, *format);
	// vips__bandalike_vec, arithmetic.c:210-254, through vips__bandup, :175-202
	const int n = left_bands > right_bands ? left_bands : right_bands;
	if ((left_bands != n && left_bands != 1) || (right_bands != n && right_bands != 1)) {
		error(domain, "not one band or %d bands", n);
		return -1;
	}
	*bands = n;
	// the output's header is ready[0]'s: the left image's own interpretation, or, banded up, that of the image it
	// was matched to
	*interpretation = left_bands == n ? left_interpretation : right_interpretation;
	*width = left_width > right_width ? left_width : right_width;
	*height = left_height > right_height ? left_height : right_height;
	return 0;
}

int vips_hip_stats_finish(double *matrix, int bands, long long pels)
{
	if (!matrix || bands < 1 || pels < 1) {
		error("stats", "bad arguments");
		return -1;
	}
	// stats.c:128-171, with its types: pels and vals are guint64
	const unsigned long long upels = (unsigned long long) pels, vals = upels * (unsigned long long) bands;
	double *row0 = matrix;
	for (int i = 0; i < COL_LAST; i++)
		row0[i] = matrix[COL_LAST + i];
	for (int b = 1; b < bands; b++) {
		const double *row = matrix + (size_t) (b + 1) * COL_LAST;
		if (row[COL_MIN] < row0[COL_MIN]) {
			row0[COL_MIN] = row[COL_MIN];
			row0[COL_XMIN] = row[COL_XMIN];
			row0[COL_YMIN] = row[COL_YMIN];
		}
		if (row[COL_MAX] > row0[COL_MAX]) {
			row0[COL_MAX] = row[COL_MAX];
			row0[COL_XMAX] = row[COL_XMAX];
			row0[COL_YMAX] = row[COL_YMAX];
		}
		row0[COL_SUM] += row[COL_SUM];
		row0[COL_SUM2] += row[COL_SUM2];
	}
	for (int y = 1; y <= bands; y++) {
		double *row = matrix + (size_t) y * COL_LAST;
		row[COL_AVG] = row[COL_SUM] / upels;
		row[COL_SD] = sqrt(fabs(row[COL_SUM2] - (row[COL_SUM] * row[COL_SUM] / upels)) / (upels - 1));
	}
	row0[COL_AVG] = row0[COL_SUM] / vals;
	row0[COL_SD] = sqrt(fabs(row0[COL_SUM2] - (row0[COL_SUM] * row0[COL_SUM] / vals)) / (vals - 1));
	return 0;
}

int vips_hip_linear_gen(const VipsHipLinear *args, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = "linear";
	if (ensure_init())
		return -1;
	if (arithmetic_window_pair(domain, in, out))
		return -1;
	ArithArgs a;
	unary_args(in, out, &a);
	int bands, format, single;
	if (vips_hip_linear_plan(args, in->bands, in->format, &bands, &format, &single, a.a, a.b))
		return -1;
	if (out->bands != bands || out->format != format) {
		error(domain, "the output must have %d bands of format %d", bands, format);
		return -1;
	}
	if ((long long) out->width * out->bands >= (1LL << 31)) {
		error(domain, "image rows too long");
		return -1;
	}
	a.single = single;
	a.a1 = (float) a.a[0];
	a.b1f = (float) a.b[0];
	return arith_run(domain, ARITH_LINEAR, in->format, out->format, a);
}

int vips_hip_invert_gen(const VipsHipRegion *in, const VipsHipRegion *out)
{
	return same_gen(ARITH_INVERT, in, out);
}

int vips_hip_abs_gen(const VipsHipRegion *in, const VipsHipRegion *out)
{
	return same_gen(ARITH_ABS, in, out);
}

int vips_hip_linear(VipsHipImage *in, VipsHipImage **out, const VipsHipLinear *args)
{
	const char *domain = "linear";
	if (enter(domain, in, out))
		return -1;
	int bands, format, single;
	if (vips_hip_linear_plan(args, in->bands, in->format, &bands, &format, &single, nullptr, nullptr))
		return -1;
	return whole_image(in, out, bands, format,
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_linear_gen(args, ri, ro); });
}

int vips_hip_invert(VipsHipImage *in, VipsHipImage **out)
{
	return same_image(ARITH_INVERT, in, out);
}

int vips_hip_abs(VipsHipImage *in, VipsHipImage **out)
{
	return same_image(ARITH_ABS, in, out);
}

int vips_hip_add(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out)
{
	return binary_image(ARITH_ADD, left, right, out);
}

int vips_hip_subtract(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out)
{
	return binary_image(ARITH_SUBTRACT, left, right, out);
}

int vips_hip_multiply(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out)
{
	return binary_image(ARITH_MULTIPLY, left, right, out);
}

int vips_hip_divide(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out)
{
	return binary_image(ARITH_DIVIDE, left, right, out);
}

int vips_hip_round_gen(int round, const VipsHipRegion *in, const VipsHipRegion *out)
{
	ArithArgs a;
	if (unary2_enter(ARITH_ROUND, in, out, &a) || check_round(round))
		return -1;
	a.round = round;
	return unary2_gen(ARITH_ROUND, in, out, in->bands, a);
}

int vips_hip_sign_gen(const VipsHipRegion *in, const VipsHipRegion *out)
{
	ArithArgs a;
	if (unary2_enter(ARITH_SIGN, in, out, &a))
		return -1;
	return unary2_gen(ARITH_SIGN, in, out, in->bands, a);
}

int vips_hip_clamp_gen(double min, double max, const VipsHipRegion *in, const VipsHipRegion *out)
{
	ArithArgs a;
	if (unary2_enter(ARITH_CLAMP, in, out, &a))
		return -1;
	a.a[0] = min;
	a.b[0] = max;
	return unary2_gen(ARITH_CLAMP, in, out, in->bands, a);
}

int vips_hip_remainder_const_gen(const double *c, int n, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = NICKNAMES[ARITH_REMAINDER_CONST];
	ArithArgs a;
	if (unary2_enter(ARITH_REMAINDER_CONST, in, out, &a))
		return -1;
	int bands;
	// (the plan writes one element a band of the output: the larger of n and the input's bands)
	std::vector<int> ci((size_t) ARITH_MAX_VECTOR + (size_t) in->bands + (size_t) (n > 0 ? n : 0));
	if (vips_hip_const_plan(domain, c, n, in->bands, in->format, &bands, nullptr, ci.data(), nullptr))
		return -1;
	for (int i = 1; i < bands; i++)
		if (ci[i] != ci[0])
			a.single = 0;
	if (!a.single && bands > ARITH_MAX_VECTOR) {
		error(domain, "vectors of more than %d elements are outside the HIP path", ARITH_MAX_VECTOR);
		return -1;
	}
	// remainder.c:277, :290: both loops read c_int
	for (int i = 0; i < ARITH_MAX_VECTOR && i < bands; i++)
		a.a[i] = (double) ci[i];
	return unary2_gen(ARITH_REMAINDER_CONST, in, out, bands, a);
}

int vips_hip_round(VipsHipImage *in, VipsHipImage **out, int round)
{
	const char *domain = NICKNAMES[ARITH_ROUND];
	if (enter(domain, in, out))
		return -1;
	if (arithmetic_noncomplex(domain, in->format) || check_round(round))
		return -1;
	// round.c:77-79: vips_unary_copy, a pointer copy
	if (in->format <= VIPS_HIP_FORMAT_INT)
		return vips_hip_cast(in, out, in->format);
	return whole_image(in, out, in->bands, in->format,
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_round_gen(round, ri, ro); });
}

int vips_hip_sign(VipsHipImage *in, VipsHipImage **out)
{
	const char *domain = NICKNAMES[ARITH_SIGN];
	if (enter(domain, in, out))
		return -1;
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	return whole_image(in, out, in->bands, vips_hip_arith_format(ARITH_SIGN, in->format), vips_hip_sign_gen);
}

int vips_hip_clamp(VipsHipImage *in, VipsHipImage **out, double min, double max)
{
	const char *domain = NICKNAMES[ARITH_CLAMP];
	if (enter(domain, in, out))
		return -1;
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	return whole_image(in, out, in->bands, in->format,
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_clamp_gen(min, max, ri, ro); });
}

int vips_hip_remainder_const(VipsHipImage *in, VipsHipImage **out, const double *c, int n)
{
	const char *domain = NICKNAMES[ARITH_REMAINDER_CONST];
	if (enter(domain, in, out))
		return -1;
	int bands;
	if (vips_hip_const_plan(domain, c, n, in->bands, in->format, &bands, nullptr, nullptr, nullptr))
		return -1;
	return whole_image(in, out, bands, in->format,
		[&](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_remainder_const_gen(c, n, ri, ro); });
}

int vips_hip_minpair(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out)
{
	return binary_image(ARITH_MINPAIR, left, right, out);
}

int vips_hip_maxpair(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out)
{
	return binary_image(ARITH_MAXPAIR, left, right, out);
}

int vips_hip_remainder(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out)
{
	return binary_image(ARITH_REMAINDER, left, right, out);
}

int vips_hip_stats(VipsHipImage *in, double *out)
{
	std::vector<double> matrix;
	if (!out) {
		error("stats", "null argument");
		return -1;
	}
	if (stats_matrix("stats", in, &matrix))
		return -1;
	memcpy(out, matrix.data(), matrix.size() * sizeof(double));
	return 0;
}

int vips_hip_avg(VipsHipImage *in, double *out)
{
	std::vector<double> matrix;
	if (!out) {
		error("avg", "null argument");
		return -1;
	}
	if (stats_matrix("avg", in, &matrix))
		return -1;
	*out = matrix[COL_AVG];
	return 0;
}

int vips_hip_deviate(VipsHipImage *in, double *out)
{
	std::vector<double> matrix;
	if (!out) {
		error("deviate", "null argument");
		return -1;
	}
	if (stats_matrix("deviate", in, &matrix))
		return -1;
	*out = matrix[COL_SD];
	return 0;
}

int vips_hip_min(VipsHipImage *in, double *out, int *x, int *y)
{
	std::vector<double> matrix;
	if (!out) {
		error("min", "null argument");
		return -1;
	}
	if (stats_matrix("min", in, &matrix, true))
		return -1;
	*out = matrix[COL_MIN];
	if (x)
		*x = (int) matrix[COL_XMIN];
	if (y)
		*y = (int) matrix[COL_YMIN];
	return 0;
}

int vips_hip_max(VipsHipImage *in, double *out, int *x, int *y)
{
	std::vector<double> matrix;
	if (!out) {
		error("max", "null argument");
		return -1;
	}
	if (stats_matrix("max", in, &matrix, true))
		return -1;
	*out = matrix[COL_MAX];
	if (x)
		*x = (int) matrix[COL_XMAX];
	if (y)
		*y = (int) matrix[COL_YMAX];
	return 0;
}

int vips_hip_arith_step(int what)
{
	return arith_tile(what);
}

} // extern "C"
