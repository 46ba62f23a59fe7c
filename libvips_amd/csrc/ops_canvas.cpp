// vips_embed, vips_gravity, vips_insert, vips_join, vips_flatten and vips_addalpha (conversion/embed.c, insert.c, join.c,
// flatten.c, addalpha.c) on images in HBM: the host side -- each class's build() restated (the identity copy, which
// extend runs, the ink, the geometry, the errors with the reference's words), the input rectangle an embed rect draws
// on, the region checks, the C ABI.  The kernels are in canvas.hip.
#include "internal.h"

#include <climits>
#include <cmath>
#include <cstring>

using namespace vh;

namespace {

// the class default of every `background` here: one zero
void background_of(int n, const double *given, int *n_out, const double **out)
{
	static const double zero[1] = { 0.0 };
	*n_out = n > 0 ? n : 1;
	*out = n > 0 ? given : zero;
}

// one axis of vips_hip_embed_need: canvas columns [left, left + n) of an image of `size` at `pos` -> [*lo, *hi] of it,
// *hi < *lo for none
void need_axis(int extend, int size, int pos, int left, int n, int *lo, int *hi)
{
	const long long t0 = (long long) left - pos, t1 = t0 + n - 1;
	if (t0 >= 0 && t1 < size) {
		*lo = (int) t0;
		*hi = (int) t1;
		return;
	}
	switch (extend) {
	case VIPS_HIP_EXTEND_COPY:
		*lo = (int) (t0 < 0 ? 0 : (t0 > size - 1 ? size - 1 : t0));
		*hi = (int) (t1 < 0 ? 0 : (t1 > size - 1 ? size - 1 : t1));
		return;
	case VIPS_HIP_EXTEND_REPEAT:
	case VIPS_HIP_EXTEND_MIRROR: {
		const bool mirror = extend == VIPS_HIP_EXTEND_MIRROR;
		const long long period = mirror ? 2LL * size : size;
		if (t1 - t0 + 1 >= period) {
			*lo = 0;
			*hi = size - 1;
			return;
		}
		long long u0 = t0 % period;
		u0 += u0 < 0 ? period : 0;
		const long long u1 = u0 + (t1 - t0);
		// the map is monotone on every stretch of `size` coordinates: the ends of the stretches bound it
		int mn = INT_MAX, mx = -1;
		for (long long k = u0 / size; k <= u1 / size; k++) {
			const long long a = k * size > u0 ? k * size : u0, b = (k + 1) * size - 1 < u1 ? (k + 1) * size - 1 : u1;
			for (const long long u : { a, b }) {
				long long m = u % period;
				if (mirror && m >= size)
					m = period - 1 - m;
				mn = m < mn ? (int) m : mn;
				mx = m > mx ? (int) m : mx;
			}
		}
		*lo = mn;
		*hi = mx;
		return;
	}
	default: {
		const long long a = t0 < 0 ? 0 : t0, b = t1 > size - 1 ? size - 1 : t1;
		*lo = (int) a;
		*hi = a <= b ? (int) b : (int) a - 1;
		return;
	}
	}
}

int canvas_mode_of(int extend)
{
	switch (extend) {
	case VIPS_HIP_EXTEND_COPY: return CANVAS_COPY;
	case VIPS_HIP_EXTEND_REPEAT: return CANVAS_REPEAT;
	case VIPS_HIP_EXTEND_MIRROR: return CANVAS_MIRROR;
	default: return CANVAS_INK;
	}
}

const int COORD_MAX = 1000000000; // the range of embed's x, y, width and height (embed.c:561-573, :643-655)
const int INSERT_COORD_MAX = 10000000; // VIPS_MAX_COORD

int embed_image(const char *domain, VipsHipImage *in, VipsHipImage **out, int x, int y, int width, int height,
	const VipsHipEmbed *args)
{
	VipsHipEmbed defaults;
	if (!args) {
		vips_hip_embed_defaults(&defaults);
		args = &defaults;
	}
	int mode, extend;
	unsigned char ink[CANVAS_MAX_PEL];
	if (vips_hip_embed_plan(domain, args, in->width, in->height, in->bands, in->format, in->interpretation, x, y, width, height,
			&mode, &extend, ink))
		return -1;
	if (mode == 0) // embed.c:360-364: vips_image_write, a pointer copy
		return vips_hip_cast(in, out, in->format);
	ImageRef o(vips_hip_image_new(width, height, in->bands, in->format, in->interpretation));
	if (!o.im)
		return -1;
	VipsHipRegion ri, ro;
	vips_hip_image_region(in, &ri);
	vips_hip_image_region(o.im, &ro);
	if (vips_hip_embed_gen(extend, ink, x, y, &ri, &ro))
		return -1;
	*out = o.release();
	return 0;
}

// arithmetic.c:76-109
int format_common(int a, int b)
{
	static const int largest[6][6] = {
		{ 0, 3, 2, 3, 4, 5 },
		{ 3, 1, 5, 3, 5, 5 },
		{ 2, 5, 2, 5, 4, 5 },
		{ 3, 3, 5, 3, 5, 5 },
		{ 4, 5, 4, 5, 4, 5 },
		{ 5, 5, 5, 5, 5, 5 },
	};
	if (a == VIPS_HIP_FORMAT_DOUBLE || b == VIPS_HIP_FORMAT_DOUBLE)
		return VIPS_HIP_FORMAT_DOUBLE;
	if (a == VIPS_HIP_FORMAT_FLOAT || b == VIPS_HIP_FORMAT_FLOAT)
		return VIPS_HIP_FORMAT_FLOAT;
	return largest[a][b];
}

// vips_insert_build with the rect of the result that is wanted (vips_join cuts its own out of the expanded canvas);
// cut[2] == 0: all of it
int insert_image(const char *domain, VipsHipImage *main, VipsHipImage *sub, VipsHipImage **out, int x, int y, int expand,
	int n_background, const double *background, const int cut[4])
{
	if (main->bands != sub->bands && main->bands != 1 && sub->bands != 1) {
		error(domain, "images must have the same number of bands, or one must be single-band");
		return -1;
	}
	if (arithmetic_noncomplex(domain, main->format) || arithmetic_noncomplex(domain, sub->format))
		return -1;
	if (x < -INSERT_COORD_MAX || x > INSERT_COORD_MAX || y < -INSERT_COORD_MAX || y > INSERT_COORD_MAX) {
		error(domain, "position out of range");
		return -1;
	}
	// vips__formatalike, vips__bandalike (arithmetic.c:111-254)
	const int format = format_common(main->format, sub->format);
	const int bands = main->bands > sub->bands ? main->bands : sub->bands;
	const int interpretation = main->bands >= sub->bands ? main->interpretation : sub->interpretation;
	ImageRef cast[2], up[2];
	VipsHipImage *im[2] = { main, sub };
	for (int i = 0; i < 2; i++) {
		if (im[i]->format != format) {
			if (vips_hip_cast(im[i], &cast[i].im, format))
				return -1;
			im[i] = cast[i].im;
		}
		if (im[i]->bands != bands) {
			if (bandup(im[i], &up[i].im, bands, interpretation))
				return -1;
			im[i] = up[i].im;
		}
	}
	// insert.c:399-430
	int m_left = 0, m_top = 0, s_left = x, s_top = y, width = im[0]->width, height = im[0]->height;
	if (expand) {
		const int left = x < 0 ? x : 0, top = y < 0 ? y : 0;
		const long long right = (long long) x + im[1]->width > im[0]->width ? (long long) x + im[1]->width : im[0]->width;
		const long long bottom = (long long) y + im[1]->height > im[0]->height ? (long long) y + im[1]->height : im[0]->height;
		if (right - left > INSERT_COORD_MAX || bottom - top > INSERT_COORD_MAX) {
			error("VipsImage", "bad dimensions");
			return -1;
		}
		width = (int) (right - left);
		height = (int) (bottom - top);
		m_left -= left;
		m_top -= top;
		s_left -= left;
		s_top -= top;
	}
	int n;
	const double *bg;
	background_of(n_background, background, &n, &bg);
	CanvasArgs a;
	memset(&a, 0, sizeof(a));
	if ((long long) bands * format_sizeof(format) > CANVAS_MAX_PEL) {
		error(domain, "pels of more than %d bytes are outside the HIP path", CANVAS_MAX_PEL);
		return -1;
	}
	if (vips_hip_vector_to_ink(bg, n, bands, format, a.ink))
		return -1;
	int rect[4] = { 0, 0, width, height };
	if (cut && cut[2] > 0)
		memcpy(rect, cut, sizeof(rect));
	if (rect[0] < 0 || rect[1] < 0 || rect[2] < 1 || rect[3] < 1 || rect[0] + rect[2] > width || rect[1] + rect[3] > height) {
		error("extract_area", "bad extract area");
		return -1;
	}
	ImageRef o(vips_hip_image_new(rect[2], rect[3], bands, format, interpretation));
	if (!o.im)
		return -1;
	a.main = (const unsigned char *) im[0]->data;
	a.main_stride = (long long) im[0]->stride;
	a.mx = m_left;
	a.my = m_top;
	a.mw = im[0]->width;
	a.mh = im[0]->height;
	a.sub = (const unsigned char *) im[1]->data;
	a.sub_stride = (long long) im[1]->stride;
	a.sx = s_left;
	a.sy = s_top;
	a.sw = im[1]->width;
	a.sh = im[1]->height;
	a.out = (unsigned char *) o.im->data;
	a.out_stride = (long long) o.im->stride;
	a.out_left = rect[0];
	a.out_top = rect[1];
	a.out_width = rect[2];
	a.out_height = rect[3];
	a.pel = bands * format_sizeof(format);
	a.mode = CANVAS_INK;
	if (canvas_run(domain, a))
		return -1;
	*out = o.release();
	return 0;
}

} // namespace

// vips__bandup (arithmetic.c:175-202) of a one-band image: every element n times, which is vips_zoom by n across of
// the same elements
int vh::bandup(VipsHipImage *in, VipsHipImage **out, int n, int interpretation)
{
	ImageRef o(vips_hip_image_new(in->width, in->height, n, in->format, interpretation));
	if (!o.im)
		return -1;
	VipsHipRegion ri, ro;
	vips_hip_image_region(in, &ri);
	vips_hip_image_region(o.im, &ro);
	ro.bands = 1;
	ro.width = ro.im_width = in->width * n;
	if (vips_hip_zoom_gen(&ri, &ro, n, 1))
		return -1;
	*out = o.release();
	return 0;
}

extern "C" {

void vips_hip_embed_defaults(VipsHipEmbed *args)
{
	if (!args)
		return;
	memset(args, 0, sizeof(*args));
	args->extend = VIPS_HIP_EXTEND_BLACK;
}

void vips_hip_flatten_defaults(VipsHipFlatten *args)
{
	if (args)
		memset(args, 0, sizeof(*args));
}

void vips_hip_insert_defaults(VipsHipInsert *args)
{
	if (args)
		memset(args, 0, sizeof(*args));
}

int vips_hip_vector_to_ink(const double *background, int n, int bands, int format, void *ink)
{
	if (!background || !ink || n < 1 || bands < 1 || format_sizeof(format) == 0 || format_iscomplex(format)) {
		error("linear", "bad arguments");
		return -1;
	}
	// vips_linear -> vips_check_vector, iofuncs/error.c:1118-1140
	if (!(n == bands || n == 1 || bands == 1)) {
		error("linear", "vector must have 1 or %d elements", bands);
		return -1;
	}
	const int es = format_sizeof(format);
	for (int z = 0; z < bands; z++)
		element_to_format(background[n == bands ? z : 0], format, (unsigned char *) ink + (size_t) z * es);
	return 0;
}

int vips_hip_embed_plan(const char *nickname, const VipsHipEmbed *args, int in_width, int in_height, int bands, int format,
	int interpretation, int x, int y, int width, int height, int *mode, int *extend_out, void *ink)
{
	const char *domain = nickname ? nickname : "embed";
	VipsHipEmbed defaults;
	if (!args) {
		vips_hip_embed_defaults(&defaults);
		args = &defaults;
	}
	if (!mode || !extend_out || !ink || in_width < 1 || in_height < 1 || bands < 1) {
		error(domain, "bad arguments");
		return -1;
	}
	if (arithmetic_noncomplex(domain, format))
		return -1;
	if (width < 1 || width > COORD_MAX || height < 1 || height > COORD_MAX || x < -COORD_MAX || x > COORD_MAX || y < -COORD_MAX ||
		y > COORD_MAX) {
		error(domain, "position or size out of range");
		return -1;
	}
	if (args->extend < VIPS_HIP_EXTEND_BLACK || args->extend > VIPS_HIP_EXTEND_BACKGROUND) {
		error(domain, "enum 'VipsExtend' has no member %d", args->extend);
		return -1;
	}
	if (args->n_background < 0 || args->n_background > VIPS_HIP_CANVAS_MAX_BACKGROUND) {
		error(domain, "background of more than %d elements", VIPS_HIP_CANVAS_MAX_BACKGROUND);
		return -1;
	}
	memset(ink, 0, CANVAS_MAX_PEL);
	*extend_out = args->extend;
	// embed.c:360-364
	if (x == 0 && y == 0 && width == in_width && height == in_height) {
		*mode = 0;
		return 0;
	}
	*mode = 1;
	// embed.c:366-368
	int extend = args->extend;
	if (!args->extend_set && args->n_background > 0)
		extend = VIPS_HIP_EXTEND_BACKGROUND;
	*extend_out = extend;
	const size_t pel = (size_t) bands * format_sizeof(format);
	if (pel > (size_t) CANVAS_MAX_PEL) {
		error(domain, "pels of more than %d bytes are outside the HIP path", CANVAS_MAX_PEL);
		return -1;
	}
	if (extend == VIPS_HIP_EXTEND_BACKGROUND) {
		int n;
		const double *bg;
		background_of(args->n_background, args->background, &n, &bg);
		if (vips_hip_vector_to_ink(bg, n, bands, format, ink))
			return -1;
	}
	if (extend == VIPS_HIP_EXTEND_REPEAT || extend == VIPS_HIP_EXTEND_MIRROR)
		return 0;
	// embed.c:454-469: the rect the image occupies, clipped to the canvas
	const long long l = x > 0 ? x : 0, t = y > 0 ? y : 0;
	const long long r = (long long) x + in_width < width ? (long long) x + in_width : width;
	const long long b = (long long) y + in_height < height ? (long long) y + in_height : height;
	if (r <= l || b <= t) {
		error(domain, "bad dimensions");
		return -1;
	}
	if (extend == VIPS_HIP_EXTEND_WHITE) {
		// vips_region_paint (iofuncs/region.c:909-956): memset for the integer formats, the value for float and double
		const int white = (int) interpretation_max_alpha(interpretation);
		if (format == VIPS_HIP_FORMAT_FLOAT) {
			const float v = (float) white;
			for (int z = 0; z < bands; z++)
				memcpy((unsigned char *) ink + (size_t) z * sizeof(v), &v, sizeof(v));
		}
		else if (format == VIPS_HIP_FORMAT_DOUBLE) {
			const double v = (double) white;
			for (int z = 0; z < bands; z++)
				memcpy((unsigned char *) ink + (size_t) z * sizeof(v), &v, sizeof(v));
		}
		else
			memset(ink, white, pel);
	}
	return 0;
}

int vips_hip_gravity_position(int direction, int in_width, int in_height, int width, int height, int *x, int *y)
{
	if (!x || !y) {
		error("gravity", "null argument");
		return -1;
	}
	// embed.c:725-783
	const int cx = (width - in_width) / 2, cy = (height - in_height) / 2;
	const int ex = width - in_width, ey = height - in_height;
	switch (direction) {
	case VIPS_HIP_COMPASS_CENTRE: *x = cx, *y = cy; break;
	case VIPS_HIP_COMPASS_NORTH: *x = cx, *y = 0; break;
	case VIPS_HIP_COMPASS_EAST: *x = ex, *y = cy; break;
	case VIPS_HIP_COMPASS_SOUTH: *x = cx, *y = ey; break;
	case VIPS_HIP_COMPASS_WEST: *x = 0, *y = cy; break;
	case VIPS_HIP_COMPASS_NORTH_EAST: *x = ex, *y = 0; break;
	case VIPS_HIP_COMPASS_SOUTH_EAST: *x = ex, *y = ey; break;
	case VIPS_HIP_COMPASS_SOUTH_WEST: *x = 0, *y = ey; break;
	case VIPS_HIP_COMPASS_NORTH_WEST: *x = 0, *y = 0; break;
	default:
		error("gravity", "enum 'VipsCompassDirection' has no member %d", direction);
		return -1;
	}
	return 0;
}

void vips_hip_embed_need(int extend, int in_width, int in_height, int x, int y, int left, int top, int width, int height,
	int need[4])
{
	if (!need)
		return;
	need[0] = need[1] = need[2] = need[3] = 0;
	if (in_width < 1 || in_height < 1 || width < 1 || height < 1)
		return;
	int x0, x1, y0, y1;
	need_axis(extend, in_width, x, left, width, &x0, &x1);
	need_axis(extend, in_height, y, top, height, &y0, &y1);
	if (x1 < x0 || y1 < y0)
		return;
	need[0] = x0;
	need[1] = y0;
	need[2] = x1 - x0 + 1;
	need[3] = y1 - y0 + 1;
}

int vips_hip_embed_gen(int extend, const void *ink, int x, int y, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = "embed";
	if (ensure_init())
		return -1;
	if (!in || !out || !ink) {
		error(domain, "null argument");
		return -1;
	}
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	if (in->bands != out->bands || in->format != out->format) {
		error(domain, "input and output must have the same bands and format");
		return -1;
	}
	if (extend < VIPS_HIP_EXTEND_BLACK || extend > VIPS_HIP_EXTEND_BACKGROUND) {
		error(domain, "enum 'VipsExtend' has no member %d", extend);
		return -1;
	}
	if (in->left < 0 || in->top < 0 || (long long) in->left + in->width > in->im_width || (long long) in->top + in->height > in->im_height ||
		out->left < 0 || out->top < 0 || (long long) out->left + out->width > out->im_width ||
		(long long) out->top + out->height > out->im_height) {
		error(domain, "region outside its image");
		return -1;
	}
	if (out->im_width > COORD_MAX || out->im_height > COORD_MAX || x < -COORD_MAX || x > COORD_MAX || y < -COORD_MAX || y > COORD_MAX) {
		error(domain, "position or size out of range");
		return -1;
	}
	if (in->data == out->data) {
		error(domain, "cannot work in place");
		return -1;
	}
	const int pel = in->bands * format_sizeof(in->format);
	if (pel > CANVAS_MAX_PEL) {
		error(domain, "pels of more than %d bytes are outside the HIP path", CANVAS_MAX_PEL);
		return -1;
	}
	int need[4];
	vips_hip_embed_need(extend, in->im_width, in->im_height, x, y, out->left, out->top, out->width, out->height, need);
	const bool all_ink = need[2] == 0 || need[3] == 0;
	if (!all_ink && (need[0] < in->left || need[1] < in->top || need[0] + need[2] > in->left + in->width ||
						need[1] + need[3] > in->top + in->height)) {
		error(domain, "input region too small");
		return -1;
	}
	CanvasArgs a;
	memset(&a, 0, sizeof(a));
	a.main = (const unsigned char *) in->data;
	a.main_stride = (long long) in->stride;
	a.mx = x;
	a.my = y;
	a.mw = in->im_width;
	a.mh = in->im_height;
	a.win_left = in->left;
	a.win_top = in->top;
	a.out = (unsigned char *) out->data;
	a.out_stride = (long long) out->stride;
	a.out_left = out->left;
	a.out_top = out->top;
	a.out_width = out->width;
	a.out_height = out->height;
	a.pel = pel;
	a.mode = canvas_mode_of(extend);
	memcpy(a.ink, ink, (size_t) pel);
	return canvas_run(domain, a);
}

int vips_hip_flatten_gen(const VipsHipRegion *in, const VipsHipRegion *out, double max_alpha, int black, const void *ink)
{
	const char *domain = "flatten";
	if (ensure_init())
		return -1;
	if (!in || !out || (!black && !ink)) {
		error(domain, "null argument");
		return -1;
	}
	if (check_region(domain, in) || check_region(domain, out))
		return -1;
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	if (in->bands < 2 || out->bands != in->bands - 1 || in->format != out->format) {
		error(domain, "the output must have the input's format and one band less");
		return -1;
	}
	if (in->width != out->width || in->height != out->height) {
		error(domain, "input and output regions must have the same size");
		return -1;
	}
	if (in->data == out->data) {
		error(domain, "cannot work in place");
		return -1;
	}
	const size_t ink_size = (size_t) out->bands * format_sizeof(in->format);
	if (ink_size > (size_t) FLATTEN_MAX_INK) {
		error(domain, "pels of more than %d bytes are outside the HIP path", FLATTEN_MAX_INK);
		return -1;
	}
	FlattenArgs a;
	memset(&a, 0, sizeof(a));
	a.in = (const unsigned char *) in->data;
	a.out = (unsigned char *) out->data;
	a.in_stride = (long long) in->stride;
	a.out_stride = (long long) out->stride;
	a.width = in->width;
	a.height = in->height;
	a.bands = in->bands;
	a.black = black != 0;
	a.max_alpha = max_alpha;
	if (!black)
		memcpy(a.ink, ink, ink_size);
	return flatten_run(domain, a, in->format);
}

int vips_hip_embed(VipsHipImage *in, VipsHipImage **out, int x, int y, int width, int height, const VipsHipEmbed *args)
{
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error("embed", "null argument");
		return -1;
	}
	return embed_image("embed", in, out, x, y, width, height, args);
}

int vips_hip_gravity(VipsHipImage *in, VipsHipImage **out, int direction, int width, int height, const VipsHipEmbed *args)
{
	if (in && bind_to(in))
		return -1;
	if (!in || !out) {
		error("gravity", "null argument");
		return -1;
	}
	int x, y;
	if (vips_hip_gravity_position(direction, in->width, in->height, width, height, &x, &y))
		return -1;
	return embed_image("gravity", in, out, x, y, width, height, args);
}

// vips_flatten_build, flatten.c:421-529
int vips_hip_flatten(VipsHipImage *in, VipsHipImage **out, const VipsHipFlatten *args)
{
	const char *domain = "flatten";
	if (in && bind_to(in))
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	VipsHipFlatten defaults;
	if (!args) {
		vips_hip_flatten_defaults(&defaults);
		args = &defaults;
	}
	if (args->n_background < 0 || args->n_background > VIPS_HIP_CANVAS_MAX_BACKGROUND) {
		error(domain, "background of more than %d elements", VIPS_HIP_CANVAS_MAX_BACKGROUND);
		return -1;
	}
	if (in->bands == 1) // "Trivial case: fall back to copy()."
		return vips_hip_cast(in, out, in->format);
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	const double max_alpha = args->max_alpha_set ? args->max_alpha : interpretation_max_alpha(in->interpretation);
	// :457-470: integer images whose max_alpha is below the format's range go through double
	ImageRef wide;
	VipsHipImage *src = in;
	const bool through_double = format_isint(in->format) && max_alpha < format_max(in->format);
	if (through_double) {
		if (vips_hip_cast(in, &wide.im, VIPS_HIP_FORMAT_DOUBLE))
			return -1;
		src = wide.im;
	}
	int n;
	const double *bg;
	background_of(args->n_background, args->background, &n, &bg);
	bool black = true;
	for (int i = 0; i < n; i++)
		if (bg[i] != 0.0)
			black = false;
	const int obands = in->bands - 1;
	unsigned char ink[FLATTEN_MAX_INK];
	memset(ink, 0, sizeof(ink));
	if (!black) {
		if ((size_t) obands * format_sizeof(src->format) > sizeof(ink)) {
			error(domain, "pels of more than %d bytes are outside the HIP path", FLATTEN_MAX_INK);
			return -1;
		}
		if (vips_hip_vector_to_ink(bg, n, obands, src->format, ink))
			return -1;
	}
	ImageRef o(vips_hip_image_new(in->width, in->height, obands, src->format, in->interpretation));
	if (!o.im)
		return -1;
	VipsHipRegion ri, ro;
	vips_hip_image_region(src, &ri);
	vips_hip_image_region(o.im, &ro);
	if (vips_hip_flatten_gen(&ri, &ro, max_alpha, black, ink))
		return -1;
	if (through_double) {
		ImageRef back;
		if (vips_hip_cast(o.im, &back.im, in->format))
			return -1;
		*out = back.release();
		return 0;
	}
	*out = o.release();
	return 0;
}

// vips_addalpha_build (addalpha.c:55-71): vips_bandjoin_const1 of max_alpha, a constant made by vips__vector_to_pels
int vips_hip_addalpha(VipsHipImage *in, VipsHipImage **out)
{
	const char *domain = "addalpha";
	if (in && bind_to(in))
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	const double max_alpha = interpretation_max_alpha(in->interpretation);
	unsigned long long alpha = 0;
	if (vips_hip_vector_to_ink(&max_alpha, 1, 1, in->format, &alpha))
		return -1;
	ImageRef o(vips_hip_image_new(in->width, in->height, in->bands + 1, in->format, in->interpretation));
	if (!o.im)
		return -1;
	if (addalpha_run(domain, (const unsigned char *) in->data, (long long) in->stride, (unsigned char *) o.im->data,
			(long long) o.im->stride, in->width, in->height, in->bands, format_sizeof(in->format), alpha))
		return -1;
	*out = o.release();
	return 0;
}

int vips_hip_insert(VipsHipImage *main, VipsHipImage *sub, VipsHipImage **out, int x, int y, const VipsHipInsert *args)
{
	const char *domain = "insert";
	if (main && bind_to(main))
		return -1;
	if (!main || !sub || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (sub->device != main->device) {
		error(domain, "the images are on different devices");
		return -1;
	}
	VipsHipInsert defaults;
	if (!args) {
		vips_hip_insert_defaults(&defaults);
		args = &defaults;
	}
	if (args->n_background < 0 || args->n_background > VIPS_HIP_CANVAS_MAX_BACKGROUND) {
		error(domain, "background of more than %d elements", VIPS_HIP_CANVAS_MAX_BACKGROUND);
		return -1;
	}
	return insert_image(domain, main, sub, out, x, y, args->expand, args->n_background, args->background, nullptr);
}

// vips_join_build, join.c:92-216: where in2 goes, vips_insert with expand, then (without `expand`) the cut
int vips_hip_join(VipsHipImage *in1, VipsHipImage *in2, VipsHipImage **out, int direction, const VipsHipInsert *args)
{
	const char *domain = "join";
	if (in1 && bind_to(in1))
		return -1;
	if (!in1 || !in2 || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (in2->device != in1->device) {
		error(domain, "the images are on different devices");
		return -1;
	}
	VipsHipInsert defaults;
	if (!args) {
		vips_hip_insert_defaults(&defaults);
		args = &defaults;
	}
	if (direction != 0 && direction != 1) {
		error(domain, "enum 'VipsDirection' has no member %d", direction);
		return -1;
	}
	if (args->align < 0 || args->align > 2) {
		error(domain, "enum 'VipsAlign' has no member %d", args->align);
		return -1;
	}
	if (args->shim < 0 || args->shim > 1000000) {
		error(domain, "shim out of range");
		return -1;
	}
	if (args->n_background < 0 || args->n_background > VIPS_HIP_CANVAS_MAX_BACKGROUND) {
		error(domain, "background of more than %d elements", VIPS_HIP_CANVAS_MAX_BACKGROUND);
		return -1;
	}
	int x = 0, y = 0;
	if (direction == 0) {
		x = in1->width + args->shim;
		y = args->align == 0 ? 0 : args->align == 1 ? in1->height / 2 - in2->height / 2 : in1->height - in2->height;
	}
	else {
		y = in1->height + args->shim;
		x = args->align == 0 ? 0 : args->align == 1 ? in1->width / 2 - in2->width / 2 : in1->width - in2->width;
	}
	int cut[4] = { 0, 0, 0, 0 };
	if (!args->expand) {
		// :164-206; the expanded canvas, for the sizes the cut keeps
		const int cw = (x + in2->width > in1->width ? x + in2->width : in1->width) - (x < 0 ? x : 0);
		const int ch = (y + in2->height > in1->height ? y + in2->height : in1->height) - (y < 0 ? y : 0);
		if (direction == 0) {
			cut[0] = 0;
			cut[1] = (0 > y ? 0 : y) - y;
			cut[2] = cw;
			cut[3] = in1->height < in2->height ? in1->height : in2->height;
		}
		else {
			cut[0] = (0 > x ? 0 : x) - x;
			cut[1] = 0;
			cut[2] = in1->width < in2->width ? in1->width : in2->width;
			cut[3] = ch;
		}
	}
	// the errors of the insert inside carry its name, as in the reference
	return insert_image("insert", in1, in2, out, x, y, 1, args->n_background, args->background, cut);
}

int vips_hip_canvas_step(int what, int pel_size)
{
	return canvas_tile(what, pel_size);
}

} // extern "C"
