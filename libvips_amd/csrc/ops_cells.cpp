// vips_arrayjoin, vips_replicate, vips_wrap, vips_grid, vips_zoom and vips_subsample (conversion/arrayjoin.c,
// replicate.c, wrap.c, grid.c, zoom.c, subsample.c) on images in HBM: the host side -- each class's build() restated
// (formats and bands made alike, the geometry, the errors with the reference's words), the input rows an output rect
// draws on, the region checks, the C ABI.  The kernels of the first four are in cells.hip; zoom and subsample run the
// region functions of upsize.hip over whole images.
#include "internal.h"

#include <climits>
#include <cstring>
#include <vector>

using namespace vh;

namespace {

const int ARG_MAX_COORD = 1000000; // the range of across, down, shim, hspacing and vspacing (arrayjoin.c, replicate.c, grid.c)

int check_pel(const char *domain, int bands, int format)
{
	if ((long long) bands * format_sizeof(format) > CANVAS_MAX_PEL) {
		error(domain, "pels of more than %d bytes are outside the HIP path", CANVAS_MAX_PEL);
		return -1;
	}
	return 0;
}

int check_window(const char *domain, const VipsHipRegion *r)
{
	if (r->left < 0 || r->top < 0 || (long long) r->left + r->width > r->im_width || (long long) r->top + r->height > r->im_height) {
		error(domain, "region outside its image");
		return -1;
	}
	return 0;
}

// what the two region functions ask of their regions
int check_pair(const char *domain, const VipsHipRegion *in, const VipsHipRegion *out)
{
	if (ensure_init())
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (check_region(domain, in) || check_region(domain, out) || arithmetic_noncomplex(domain, in->format))
		return -1;
	if (in->bands != out->bands || in->format != out->format) {
		error(domain, "input and output must have the same bands and format");
		return -1;
	}
	if (check_window(domain, in) || check_window(domain, out) || check_pel(domain, in->bands, in->format))
		return -1;
	if (in->data == out->data) {
		error(domain, "cannot work in place");
		return -1;
	}
	return 0;
}

bool holds(const VipsHipRegion *in, const int need[4])
{
	return need[0] >= in->left && need[1] >= in->top && need[0] + need[2] <= in->left + in->width &&
		need[1] + need[3] <= in->top + in->height;
}

// one axis of vips_hip_replicate_need: `n` output positions from `left` of a period of `size` that the output's
// position 0 lies `org` into
void period_axis(int size, int org, int left, int n, int *lo, int *len)
{
	const long long u0 = ((long long) left + org) % size;
	if (u0 + n <= size) {
		*lo = (int) u0;
		*len = n;
	}
	else {
		*lo = 0;
		*len = size;
	}
}

void fill_out(CellsArgs *a, const VipsHipRegion *out)
{
	a->out = (unsigned char *) out->data;
	a->out_stride = (long long) out->stride;
	a->out_left = out->left;
	a->out_top = out->top;
	a->out_width = out->width;
	a->out_height = out->height;
}

void fill_src(CellsArgs *a, const VipsHipRegion *in)
{
	a->src = (const unsigned char *) in->data;
	a->src_stride = (long long) in->stride;
	a->sw = in->im_width;
	a->sh = in->im_height;
	a->win_left = in->left;
	a->win_top = in->top;
	a->pel = in->bands * format_sizeof(in->format);
}

// a one-image operation whose result has the input's bands, format and interpretation
template <typename Gen>
int whole_image(VipsHipImage *in, VipsHipImage **out, long long width, long long height, const char *domain, Gen gen)
{
	if (width > INT_MAX || height > INT_MAX) {
		error(domain, "output size overflows an int");
		return -1;
	}
	ImageRef o(vips_hip_image_new((int) width, (int) height, in->bands, in->format, in->interpretation));
	if (!o.im)
		return -1;
	VipsHipRegion ri, ro;
	vips_hip_image_region(in, &ri);
	vips_hip_image_region(o.im, &ro);
	if (gen(&ri, &ro))
		return -1;
	*out = o.release();
	return 0;
}

int check_align(const char *domain, int align)
{
	if (align < 0 || align > 2) {
		error(domain, "enum 'VipsAlign' has no member %d", align);
		return -1;
	}
	return 0;
}

int check_arrayjoin_args(const char *domain, const VipsHipArrayjoin *args)
{
	if (check_align(domain, args->halign) || check_align(domain, args->valign))
		return -1;
	if (args->across < 0 || args->across > ARG_MAX_COORD || args->shim < 0 || args->shim > ARG_MAX_COORD || args->hspacing < 0 ||
		args->hspacing > ARG_MAX_COORD || args->vspacing < 0 || args->vspacing > ARG_MAX_COORD) {
		error(domain, "across, shim or spacing out of range");
		return -1;
	}
	if (args->n_background < 0 || args->n_background > VIPS_HIP_CANVAS_MAX_BACKGROUND) {
		error(domain, "background of more than %d elements", VIPS_HIP_CANVAS_MAX_BACKGROUND);
		return -1;
	}
	return 0;
}

} // namespace

extern "C" {

void vips_hip_arrayjoin_defaults(VipsHipArrayjoin *args)
{
	if (args)
		memset(args, 0, sizeof(*args));
}

int vips_hip_arrayjoin_plan(const VipsHipArrayjoin *args, int n, const int *widths, const int *heights, int *out_width,
	int *out_height, int *across_out, int *rects, int *offsets)
{
	const char *domain = "arrayjoin";
	VipsHipArrayjoin defaults;
	if (!args) {
		vips_hip_arrayjoin_defaults(&defaults);
		args = &defaults;
	}
	if (!widths || !heights || !out_width || !out_height || !across_out || !rects || !offsets) {
		error(domain, "null argument");
		return -1;
	}
	if (n < 1) { // arrayjoin.c:205-208
		error(domain, "no input images");
		return -1;
	}
	if (check_arrayjoin_args(domain, args))
		return -1;
	// :231-251
	int hspacing = widths[0], vspacing = heights[0];
	for (int i = 0; i < n; i++) {
		if (widths[i] < 1 || heights[i] < 1) {
			error(domain, "bad image size");
			return -1;
		}
		hspacing = widths[i] > hspacing ? widths[i] : hspacing;
		vspacing = heights[i] > vspacing ? heights[i] : vspacing;
	}
	if (args->hspacing)
		hspacing = args->hspacing;
	if (args->vspacing)
		vspacing = args->vspacing;
	const int across = args->across ? args->across : n;
	// :255-262
	const int down = (n + across - 1) / across;
	const int shim = args->shim;
	const long long width = (long long) hspacing * across + (long long) shim * (across - 1);
	const long long height = (long long) vspacing * down + (long long) shim * (down - 1);
	if (width > INT_MAX || height > INT_MAX) {
		error(domain, "output size overflows an int");
		return -1;
	}
	for (int i = 0; i < n; i++) {
		// :267-290
		const int x = i % across, y = i / across;
		int *r = rects + 4 * i;
		r[0] = x * (hspacing + shim);
		r[1] = y * (vspacing + shim);
		r[2] = hspacing + (x != across - 1 ? shim : 0);
		r[3] = vspacing + (y != down - 1 ? shim : 0);
		if (i == n - 1)
			r[2] = (int) width - r[0];
		// :311-345
		const int slack_x = hspacing - widths[i], slack_y = vspacing - heights[i];
		offsets[2 * i] = args->halign == 0 ? 0 : args->halign == 1 ? slack_x / 2 : slack_x;
		offsets[2 * i + 1] = args->valign == 0 ? 0 : args->valign == 1 ? slack_y / 2 : slack_y;
	}
	*out_width = (int) width;
	*out_height = (int) height;
	*across_out = across;
	return 0;
}

int vips_hip_arrayjoin(VipsHipImage **in, int n, VipsHipImage **out, const VipsHipArrayjoin *args)
{
	const char *domain = "arrayjoin";
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (n < 1) {
		error(domain, "no input images");
		return -1;
	}
	for (int i = 0; i < n; i++)
		if (!in[i]) {
			error(domain, "null argument");
			return -1;
		}
	if (bind_to(in[0]))
		return -1;
	VipsHipArrayjoin defaults;
	if (!args) {
		vips_hip_arrayjoin_defaults(&defaults);
		args = &defaults;
	}
	if (check_arrayjoin_args(domain, args))
		return -1;
	for (int i = 0; i < n; i++) {
		if (in[i]->device != in[0]->device) {
			error(domain, "the images are on different devices");
			return -1;
		}
		if (arithmetic_noncomplex(domain, in[i]->format))
			return -1;
	}
	static const double zero[1] = { 0.0 };
	const int n_background = args->n_background > 0 ? args->n_background : 1;
	const double *background = args->n_background > 0 ? args->background : zero;
	// vips__formatalike_vec (arithmetic.c:111-137), vips__bandalike_vec (:210-254) with the background's length as the
	// least: the tag of the last image that has the most bands goes to the images that are banded up
	int format = in[0]->format, bands = n_background, interpretation = -1;
	for (int i = 0; i < n; i++) {
		format = format_common(format, in[i]->format);
		if (in[i]->bands >= bands) {
			bands = in[i]->bands;
			interpretation = in[i]->interpretation;
		}
	}
	for (int i = 0; i < n; i++)
		if (in[i]->bands != bands && in[i]->bands != 1) {
			error(domain, "not one band or %d bands", bands);
			return -1;
		}
	if (check_pel(domain, bands, format))
		return -1;
	std::vector<ImageRef> cast(n), up(n);
	std::vector<VipsHipImage *> im(in, in + n);
	for (int i = 0; i < n; i++) {
		if (im[i]->format != format) {
			if (vips_hip_cast(im[i], &cast[i].im, format))
				return -1;
			im[i] = cast[i].im;
		}
		if (im[i]->bands != bands) {
			if (bandup(im[i], &up[i].im, bands, interpretation >= 0 ? interpretation : im[i]->interpretation))
				return -1;
			im[i] = up[i].im;
		}
	}
	std::vector<int> widths(n), heights(n), rects(4 * (size_t) n), offsets(2 * (size_t) n);
	for (int i = 0; i < n; i++) {
		widths[i] = im[i]->width;
		heights[i] = im[i]->height;
	}
	int width, height, across;
	if (vips_hip_arrayjoin_plan(args, n, widths.data(), heights.data(), &width, &height, &across, rects.data(), offsets.data()))
		return -1;
	CellsArgs a;
	memset(&a, 0, sizeof(a));
	// :350-354: the ink is made by each image's vips_embed, and an embed that changes nothing is a copy that never looks
	// at its background (embed.c:360-364): a vector of the wrong length is an error only where some rect shows ink
	bool inked = false;
	for (int i = 0; i < n; i++)
		inked |= offsets[2 * i] != 0 || offsets[2 * i + 1] != 0 || rects[4 * i + 2] != widths[i] || rects[4 * i + 3] != heights[i];
	if (inked && vips_hip_vector_to_ink(background, n_background, bands, format, a.ink))
		return -1;
	// :357-362: the header is the first image's
	ImageRef o(vips_hip_image_new(width, height, bands, format, im[0]->interpretation));
	if (!o.im)
		return -1;
	const int pel = bands * format_sizeof(format);
	std::vector<CellDesc> table(n);
	unsigned long long starts = 0;
	for (int i = 0; i < n; i++) {
		if ((long long) im[i]->width * pel >= (1LL << 31)) {
			error(domain, "image rows too long");
			return -1;
		}
		table[i].base = (const unsigned char *) im[i]->data;
		table[i].stride = (long long) im[i]->stride;
		table[i].x0 = rects[4 * i] + offsets[2 * i];
		table[i].y0 = rects[4 * i + 1] + offsets[2 * i + 1];
		table[i].w = im[i]->width;
		table[i].h = im[i]->height;
		starts |= (unsigned long long) (uintptr_t) im[i]->data | (unsigned long long) im[i]->stride;
	}
	// (the upload waits for the stream: the table is this call's own and goes back to the pool behind the launch)
	void *d_table = upload(table.data(), table.size() * sizeof(CellDesc));
	if (!d_table)
		return -1;
	VipsHipRegion ro;
	vips_hip_image_region(o.im, &ro);
	fill_out(&a, &ro);
	a.table = (const CellDesc *) d_table;
	a.mode = CELLS_TABLE;
	a.n = n;
	a.across = across;
	// arrayjoin.c:95-96: a cell is the spacing and the shim; width = hspacing * across + shim * (across - 1)
	a.cell_w = (int) (((long long) width + args->shim) / across);
	a.cell_h = (int) (((long long) height + args->shim) / ((n + across - 1) / across));
	a.pel = pel;
	const int result = cells_run(domain, a, starts);
	vips_hip_free(d_table);
	if (result)
		return -1;
	*out = o.release();
	return 0;
}

void vips_hip_replicate_need(int in_width, int in_height, int x0, int y0, int left, int top, int width, int height, int need[4])
{
	if (!need)
		return;
	need[0] = need[1] = need[2] = need[3] = 0;
	if (in_width < 1 || in_height < 1 || width < 1 || height < 1 || left < 0 || top < 0 || x0 < 0 || y0 < 0)
		return;
	period_axis(in_width, x0, left, width, &need[0], &need[2]);
	period_axis(in_height, y0, top, height, &need[1], &need[3]);
}

void vips_hip_grid_need(int in_width, int in_height, int tile_height, int across, int left, int top, int width, int height,
	int need[4])
{
	if (!need)
		return;
	need[0] = need[1] = need[2] = need[3] = 0;
	if (in_width < 1 || in_height < 1 || tile_height < 1 || across < 1 || width < 1 || height < 1 || left < 0 || top < 0)
		return;
	// grid.c:103,136: tile (tx, ty) is rows (ty * across + tx) * tile_height ... of the strip
	const long long tx0 = left / in_width, tx1 = ((long long) left + width - 1) / in_width;
	const long long ty0 = top / tile_height, ty1 = ((long long) top + height - 1) / tile_height;
	const long long first = (ty0 * across + tx0) * tile_height + (top - ty0 * tile_height);
	const long long last = (ty1 * across + tx1) * tile_height + ((long long) top + height - 1 - ty1 * tile_height);
	if (last >= in_height || tx1 >= across)
		return;
	need[0] = tx0 == tx1 ? (int) (left - tx0 * in_width) : 0;
	need[2] = tx0 == tx1 ? width : in_width;
	need[1] = (int) first;
	need[3] = (int) (last - first + 1);
}

int vips_hip_replicate_gen(int x0, int y0, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = "replicate";
	if (check_pair(domain, in, out))
		return -1;
	if (x0 < 0 || x0 > in->im_width || y0 < 0 || y0 > in->im_height) {
		error(domain, "offset outside the image");
		return -1;
	}
	int need[4];
	vips_hip_replicate_need(in->im_width, in->im_height, x0, y0, out->left, out->top, out->width, out->height, need);
	if (!holds(in, need)) {
		error(domain, "input region too small");
		return -1;
	}
	CellsArgs a;
	memset(&a, 0, sizeof(a));
	fill_src(&a, in);
	fill_out(&a, out);
	a.mode = CELLS_REPEAT;
	a.cell_w = in->im_width;
	a.cell_h = in->im_height;
	a.org_x = x0;
	a.org_y = y0;
	return cells_run(domain, a, (unsigned long long) (uintptr_t) in->data | (unsigned long long) in->stride);
}

int vips_hip_grid_gen(int tile_height, int across, const VipsHipRegion *in, const VipsHipRegion *out)
{
	const char *domain = "grid";
	if (check_pair(domain, in, out))
		return -1;
	if (tile_height < 1 || across < 1) {
		error(domain, "bad grid geometry");
		return -1;
	}
	int need[4];
	vips_hip_grid_need(in->im_width, in->im_height, tile_height, across, out->left, out->top, out->width, out->height, need);
	if (need[2] == 0 || need[3] == 0) {
		error(domain, "bad grid geometry");
		return -1;
	}
	if (!holds(in, need)) {
		error(domain, "input region too small");
		return -1;
	}
	CellsArgs a;
	memset(&a, 0, sizeof(a));
	fill_src(&a, in);
	fill_out(&a, out);
	a.mode = CELLS_GRID;
	a.across = across;
	a.cell_w = in->im_width;
	a.cell_h = tile_height;
	return cells_run(domain, a, (unsigned long long) (uintptr_t) in->data | (unsigned long long) in->stride);
}

int vips_hip_replicate(VipsHipImage *in, VipsHipImage **out, int across, int down)
{
	const char *domain = "replicate";
	if (in && bind_to(in))
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (across < 1 || across > ARG_MAX_COORD || down < 1 || down > ARG_MAX_COORD) {
		error(domain, "across and down must be 1 .. %d", ARG_MAX_COORD);
		return -1;
	}
	if (arithmetic_noncomplex(domain, in->format) || check_pel(domain, in->bands, in->format))
		return -1;
	return whole_image(in, out, (long long) in->width * across, (long long) in->height * down, domain,
		[](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_replicate_gen(0, 0, ri, ro); });
}

int vips_hip_wrap(VipsHipImage *in, VipsHipImage **out, int x, int y, int x_set, int y_set)
{
	const char *domain = "wrap";
	if (in && bind_to(in))
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (arithmetic_noncomplex(domain, in->format) || check_pel(domain, in->bands, in->format))
		return -1;
	// wrap.c:78-91; INT_MIN has no negative
	if (x == INT_MIN || y == INT_MIN) {
		error(domain, "position out of range");
		return -1;
	}
	if (!x_set)
		x = in->width / 2;
	if (!y_set)
		y = in->height / 2;
	const int x0 = x < 0 ? -x % in->width : in->width - x % in->width;
	const int y0 = y < 0 ? -y % in->height : in->height - y % in->height;
	return whole_image(in, out, in->width, in->height, domain,
		[x0, y0](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_replicate_gen(x0, y0, ri, ro); });
}

int vips_hip_grid(VipsHipImage *in, VipsHipImage **out, int tile_height, int across, int down)
{
	const char *domain = "grid";
	if (in && bind_to(in))
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (tile_height < 1 || tile_height > 10000000 || across < 1 || across > 10000000 || down < 1 || down > 10000000) {
		error(domain, "tile_height, across and down must be 1 .. 10000000");
		return -1;
	}
	if (arithmetic_noncomplex(domain, in->format) || check_pel(domain, in->bands, in->format))
		return -1;
	// grid.c:162-167
	if (in->height % tile_height != 0 || in->height / tile_height != (long long) across * down) {
		error(domain, "bad grid geometry");
		return -1;
	}
	return whole_image(in, out, (long long) in->width * across, (long long) tile_height * down, domain,
		[tile_height, across](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_grid_gen(tile_height, across, ri, ro); });
}

int vips_hip_zoom(VipsHipImage *in, VipsHipImage **out, int xfac, int yfac)
{
	const char *domain = "zoom";
	if (in && bind_to(in))
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (xfac < 1 || yfac < 1) {
		error(domain, "zoom factors should be >= 1");
		return -1;
	}
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	// zoom.c:322-329
	if ((double) in->width * xfac > (double) INT_MAX / 2 || (double) in->height * yfac > (double) INT_MAX / 2) {
		error(domain, "zoom factors too large");
		return -1;
	}
	if (xfac == 1 && yfac == 1) // :330-332: vips_image_write
		return vips_hip_cast(in, out, in->format);
	return whole_image(in, out, (long long) in->width * xfac, (long long) in->height * yfac, domain,
		[xfac, yfac](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_zoom_gen(ri, ro, xfac, yfac); });
}

int vips_hip_subsample(VipsHipImage *in, VipsHipImage **out, int xfac, int yfac)
{
	const char *domain = "subsample";
	if (in && bind_to(in))
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	if (xfac < 1 || yfac < 1) {
		error(domain, "factors should be positive");
		return -1;
	}
	if (arithmetic_noncomplex(domain, in->format))
		return -1;
	if (xfac == 1 && yfac == 1) // subsample.c:207-209: vips_image_write
		return vips_hip_cast(in, out, in->format);
	// :223-230
	if (in->width / xfac <= 0 || in->height / yfac <= 0) {
		error(domain, "image has shrunk to nothing");
		return -1;
	}
	return whole_image(in, out, in->width / xfac, in->height / yfac, domain,
		[xfac, yfac](const VipsHipRegion *ri, const VipsHipRegion *ro) { return vips_hip_subsample_gen(ri, ro, xfac, yfac); });
}

int vips_hip_cells_step(int what, int pel_size)
{
	return cells_tile(what, pel_size);
}

} // extern "C"
