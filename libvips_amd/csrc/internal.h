// Internal declarations shared by the HIP translation units of libvipship.so.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <memory>

#include "vips_hip.h"

namespace vh {

// iofuncs/error.c shaped error log: "domain: message\n" appended to a
// thread-local buffer; every failing entry point returns -1 after calling it.
void error(const char *domain, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int hip_failed(hipError_t err, const char *what);

#define VH_CHECK(expr) \
	do { \
		hipError_t vh_err_ = (expr); \
		if (vh_err_ != hipSuccess) \
			return vh::hip_failed(vh_err_, #expr); \
	} while (0)

#define VH_CHECK_NULL(expr) \
	do { \
		hipError_t vh_err_ = (expr); \
		if (vh_err_ != hipSuccess) { \
			vh::hip_failed(vh_err_, #expr); \
			return nullptr; \
		} \
	} while (0)

// Make sure a device has been selected for this thread (vips_hip_init(0) on
// first use) -- returns -1 with an error when no GPU is present.
int ensure_init();

// The device the calling thread is bound to (-1: none yet).
int current_device();

hipStream_t stream();
// Synchronise and destroy the calling thread's own stream (threads the library starts itself).
void release_thread_stream();

// The calling thread launches on `s` while this lives (nullptr: no change).  For work the
// library spreads over a second stream itself; whoever does so orders the streams with events
// and keeps pool blocks both streams touch alive until both are synchronised.
struct ScopedStream {
	explicit ScopedStream(hipStream_t s);
	~ScopedStream();
	hipStream_t saved;
	int slot; // the device slot `saved` came from
	bool saved_external, active;
};

// vips_hip_get_exact_float() is 1 on the calling thread while this lives (see runtime.cpp).
struct ScopedExactFloat {
	ScopedExactFloat();
	~ScopedExactFloat();
};

// Kernel gates: VIPS_GATE_START/STOP analogue around a launch.
struct Gate {
	explicit Gate(const char *name);
	~Gate();
	const char *name;
	hipEvent_t start;
	bool active;
};

// sizeof one band element
static inline int format_sizeof(int format)
{
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR:
	case VIPS_HIP_FORMAT_CHAR:
		return 1;
	case VIPS_HIP_FORMAT_USHORT:
	case VIPS_HIP_FORMAT_SHORT:
		return 2;
	case VIPS_HIP_FORMAT_UINT:
	case VIPS_HIP_FORMAT_INT:
	case VIPS_HIP_FORMAT_FLOAT:
		return 4;
	case VIPS_HIP_FORMAT_COMPLEX:
	case VIPS_HIP_FORMAT_DOUBLE:
		return 8;
	case VIPS_HIP_FORMAT_DPCOMPLEX:
		return 16;
	default:
		return 0;
	}
}

static inline bool format_iscomplex(int format)
{
	return format == VIPS_HIP_FORMAT_COMPLEX || format == VIPS_HIP_FORMAT_DPCOMPLEX;
}

static inline bool format_isint(int format)
{
	return format >= VIPS_HIP_FORMAT_UCHAR && format <= VIPS_HIP_FORMAT_INT;
}

// Complex images are processed as twice as many bands of the real type
// (reduceh.cpp:227-228, shrinkh.c:162-163, convi.c:770-771).
static inline int format_real(int format)
{
	if (format == VIPS_HIP_FORMAT_COMPLEX)
		return VIPS_HIP_FORMAT_FLOAT;
	if (format == VIPS_HIP_FORMAT_DPCOMPLEX)
		return VIPS_HIP_FORMAT_DOUBLE;
	return format;
}

static inline int region_elems_per_pel(const VipsHipRegion *r)
{
	return r->bands * (format_iscomplex(r->format) ? 2 : 1);
}

// Common checks on a pair of regions handed to a gen.
int check_region(const char *domain, const VipsHipRegion *r);

// A plan handle's device tables live on ONE device: the device of the thread that first runs
// it (*device < 0: taken now).  Running it from a thread bound to another device fails loudly.
int plan_device(const char *domain, std::atomic<int> *device);

// Small device-resident table upload with caching handled by the callers.
void *upload(const void *host, size_t size);

} // namespace vh

// The image object (layer 3).
struct _VipsHipImage {
	void *data;
	int device = -1; // the device the pixels live on
	int width, height, bands, format, interpretation;
	size_t stride;
	bool owns; // data came from the pool
	// library memory is shared between image objects (vips_copy-style no-op results): the
	// last holder returns it to the pool
	std::shared_ptr<void> hold;
	// EXIF-style orientation, 1 .. 8; 0: the image has none (read as 1, vips_image_get_orientation, iofuncs/header.c).
	// Set by the JPEG and .v loaders and vips_hip_image_set_orientation, carried by vips_hip_rot / vips_hip_flip,
	// cleared by vips_hip_autorot; every other operation's result has none.
	int orientation = 0;
};

namespace vh {
// Run where the data lives: make sure a device is selected and bind the calling thread to the
// device `image` is on (every image-level operation starts with this).
int bind_to(const _VipsHipImage *image);
// A reference to an image that is dropped on the way out of a scope, unless it is released to the caller.
struct ImageRef {
	VipsHipImage *im;
	explicit ImageRef(VipsHipImage *i = nullptr)
		: im(i)
	{
	}
	~ImageRef() { vips_hip_image_unref(im); }
	VipsHipImage *release()
	{
		VipsHipImage *t = im;
		im = nullptr;
		return t;
	}
};
// ... device memory from the pool (nullptr for no bytes, and when the pool fails)
struct DeviceBlock {
	void *p;
	explicit DeviceBlock(size_t size)
		: p(size ? vips_hip_malloc(size) : nullptr)
	{
	}
	~DeviceBlock() { vips_hip_free(p); }
};
// A second image object on the same pixels (library-owned images only; nullptr otherwise).  It has no orientation.
_VipsHipImage *image_share(const _VipsHipImage *in);
// How a one-image entry point starts: bound to the input's device, then the null check
static inline int enter(const char *domain, _VipsHipImage *in, void *out)
{
	if (in && bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error(domain, "null argument");
		return -1;
	}
	return 0;
}
// ... and how it ends when it is a generate function over whole images: the output has the input's size and
// interpretation; gen(in, out) is the region function with its other arguments bound
template <typename Gen>
static inline int whole_image(_VipsHipImage *in, _VipsHipImage **out, int bands, int format, Gen gen)
{
	ImageRef o(vips_hip_image_new(in->width, in->height, bands, format, in->interpretation));
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
// rot.hip: out = in turned and / or mirrored in one launch; op is a sum of ROT_OP_*
enum { ROT_OP_TRANSPOSE = 1, ROT_OP_FLIPX = 2, ROT_OP_FLIPY = 4 };
int rot_op_gen(const char *domain, int op, const VipsHipRegion *in, const VipsHipRegion *out);
// the operation vips_autorot runs for an orientation (autorot.c:119-160 folded: a turn and the flip behind it are
// one operation here); 0 for orientations that change nothing
int orientation_op(int orientation);
// hist.hip: the histograms of n (1 .. HIST_MAX_RECTS) rectangles of a uchar image of 1 .. 4 bands, ONE launch.
// Rectangle k's counts are ADDED to counters[k * 256 * bands + value * bands + band] (device memory, zero before
// the first launch that uses them): the pel order of vips_hist_find's output.
struct HistRect {
	int left, top, width, height;
};
constexpr int HIST_MAX_RECTS = 6;
int hist_rects(const char *domain, const _VipsHipImage *in, const HistRect *rects, int n, unsigned int *counters);
// rank.hip, morph.hip: the neighbourhood filters on checked regions (ops_morphology.cpp checks them and fills the
// geometry of NbArgs, nbhd_tile.h; the kernels' files set the rest).  `mask` holds 0, 128 and 255.  *_tile: 0 the
// elements of a row a block makes, 1 its rows (morph_tile 2: the largest mask side).
struct NbArgs {
	const unsigned char *in;
	unsigned char *out;
	long long in_stride, out_stride;          // bytes
	int in_left, in_top, in_width, in_height; // the input window, pels of the whole image
	int im_width, im_height;
	int out_left, out_top, out_width, out_height; // `out` points at pel (out_left, out_top)
	int bands;        // elements a pel
	int win_w, win_h; // the neighbourhood, pels; its origin is (win_w / 2, win_h / 2)
	int lds_row;      // bytes of a staged row, a multiple of 16
	int index;        // rank: the index-th smallest
	unsigned int key_xor;
};
// hist.hip: vips_maplut of a uchar image through a packed table in device memory (ops_histogram.cpp checks everything
// and packs it): entry (v, z) -- index v < n, table z < tables -- is the `es` bytes at table[(v * tables + z) * es].  Output
// element o of a row comes from input element o / spread through table o % tables (tables 1: every element through
// the one table; spread > 1: a one-band image through `spread` tables).
constexpr int MAPLUT_TABLE_MAX = 256 * 4 * 8; // bytes: what the kernel keeps in LDS
struct MaplutArgs {
	const unsigned char *in;
	unsigned char *out;
	const unsigned char *table; // device memory, n * tables * es bytes
	long long in_stride, out_stride; // bytes
	int in_elems;  // of a row of the input
	int height;
	int n, tables, es, spread;
};
int maplut_run(const char *domain, MaplutArgs a);
// hist_local.hip: vips_hist_local and vips_stdif on checked regions of uchar images (ops_histogram.cpp, nb_geometry).
// hist_local_tile: 0 the pels of a run, 1 the rows a block of the sliding kernel makes, 2 the largest window side,
// 3 the lanes of a block that share a row, 4 the largest window area of the counting kernel.
int hist_local_run(const char *domain, NbArgs a, int max_slope);
int hist_local_tile(int what);
struct StdifArgs {
	NbArgs nb;
	double f1, f2, f3, s0, b; // stdif.c:170-172: a * m0, 1 - a, b * s0
	int rows;                 // output rows a block makes
};
int stdif_run(const char *domain, StdifArgs a);
int stdif_tile(int what); // 0 / 1: elements of a row / rows (at most) a block makes, 2: the largest window area
int rank_run(const char *domain, NbArgs a, int format);
int morph_run(const char *domain, NbArgs a, const unsigned char *mask, int dilate);
int rank_tile(int what);
int morph_tile(int what);
// ops_morphology.cpp: the checks every neighbourhood gen makes on its pair of regions, and the geometry of the launch:
// @in must hold the out rect grown by the window (origin win_w / 2, win_h / 2) and clipped to the image.
int nb_geometry(const char *domain, const VipsHipRegion *in, const VipsHipRegion *out, int win_w, int win_h, NbArgs *a);
// edge.hip: the fused uchar kernel of vips_sobel and its siblings on checked regions (ops_edge.cpp), `mask` and
// `mask90` 3 x 3 in raster order; edge_u8_fits: the tile of so wide a pel fits the kernel's LDS; edge_tile as above
// (2: the widest pel that fits).  edge_combine_run: the general tier's tail on the two convolutions' rows.
int edge_u8_run(const char *domain, NbArgs a, const int *mask, const int *mask90);
int edge_u8_fits(int bands);
int edge_tile(int what);
int edge_combine_run(const char *domain, const void *c1, long long c1_stride, const void *c2, long long c2_stride, void *out,
	long long out_stride, long long elems, int height, int is_float);
// ... of vips_compass for uchar, precision integer, 3 x 3: `masks` n x 9 ints, `mult` how often each runs, `combine` a
// VipsHipCombine; compass_u8_takes: the kernel takes these masks.  compass_combine_run: the general tier's tail on n
// planes of convolutions in `format`.
int compass_u8_takes(int bands, const int *masks, int n, int scale);
int compass_u8_run(const char *domain, NbArgs a, const int *masks, const int *mult, int n, int scale, int offset, int combine);
int compass_combine_run(const char *domain, const void *in, long long in_stride, long long plane, int n, int times, int format,
	int combine, void *out, long long out_stride, long long elems, int height);
// ... of vips_canny behind its blur: the gradient pair, the polar image and the thinning on a checked window of the
// blurred image (ops_edge.cpp checks it and fills everything but the table).  canny_tile: 0 / 1 the pels / rows a block
// makes, 2 the widest pel.
constexpr int CANNY_TABLE = 256; // bytes: the atan2 table of the uchar path
struct CannyArgs {
	const unsigned char *in; // the blurred image's window
	unsigned char *out;
	long long in_stride, out_stride;          // bytes
	int in_left, in_top, in_width, in_height; // the window, pels of the whole image
	int im_width, im_height;
	int out_left, out_top, out_width, out_height; // `out` points at pel (out_left, out_top)
	int bands;
	int format;             // of the blurred image: uchar takes the integer kernel, everything else the float one
	unsigned int *marginal; // float kernel: the counter behind vips_hip_canny_marginal
	unsigned int atan2_table[CANNY_TABLE / 4]; // vips_canny_polar_atan2 (uchar kernel)
};
int canny_run(const char *domain, CannyArgs a, const unsigned char *table);
int canny_tile(int what);
// affine.hip: vips_affine_gen on checked regions (ops_affine.cpp checks them and fills everything).  Coordinates are
// the reference's: ox = (double) (rect start + oarea_left) - odx, x = ia * ox + ib * oy, -= tidx (idx less the
// one-pel embed), += window_offset, then += ia per pixel from the rect's left edge, rects starting at multiples of
// tile_width (0: whole rows; the x of a column then comes from a table made on the host and y does not move).
struct AffineArgs {
	const unsigned char *in;
	unsigned char *out;
	long long in_stride, out_stride;          // bytes
	int in_left, in_top, in_width, in_height; // the input window, pels of the whole image; in_width == 0: no window
	int im_width, im_height;                  // the whole input image
	int out_left, out_top, out_width, out_height; // `out` points at pel (out_left, out_top) of the output image
	int bands;                                // elements a pel
	int window_offset;
	int extend;     // VipsHipExtend
	int tile_width; // 0: whole rows
	int oarea_left, oarea_top;
	double ia, ib, ic, id, odx, ody, tidx, tidy;
	const double *tabx; // tile_width == 0: the x of output column out_left + i
	const void *tables; // BicubicTables, interp_device.h
	unsigned char ink[VIPS_HIP_AFFINE_MAX_PEL];  // the pel of what lies outside the clip rectangle
	unsigned char fill[VIPS_HIP_AFFINE_MAX_PEL]; // the pel round the image under extend black / white / background
};
// format: uchar .. int or float; interpolate: VipsHipInterpolate
int affine_run(const char *domain, AffineArgs a, int format, int interpolate);
// ops_affine.cpp: what vips_affine and vips_mapim share on the host.  resample_check: the interpolator, the extend and
// the image format are ones the path takes (refused by name otherwise).  resample_pels: the ink and the embed's fill
// pel of vips__vector_to_ink and embed.c:270-298, the premultiply chain's decision and the stencil
// (interpolate.c:150-167); resample_fill_premultiply: the chain's fill pel through vips_premultiply, once.
struct ResamplePels {
	bool chain;  // premultiply -> resample -> unpremultiply -> cast
	int kformat; // the format of the image the kernel resamples
	int window_size, window_offset;
	bool fill_ready;
	unsigned char ink[VIPS_HIP_AFFINE_MAX_PEL];
	unsigned char fill[VIPS_HIP_AFFINE_MAX_PEL]; // in the image's own format until resample_fill_premultiply
};
int resample_check(const char *domain, int interpolate, int extend, int format);
int resample_pels(const char *domain, int interpolate, int extend, int premultiplied, int n_background, const double *background,
	int bands, int format, int interpretation, ResamplePels *p);
int resample_fill_premultiply(const char *domain, ResamplePels *p, int bands, int format, int interpretation);
// ... one axis of the embedded rect [e0, e1] as pels of the image: what EmbedFetch (interp_device.h) reads for it
void embedded_axis_to_image(int extend, int off, int size, int e0, int e1, int *p0, int *p1);
// mapim.hip: vips_mapim_gen on checked regions (ops_mapim.cpp checks them and fills everything): output pel (i, y) of
// the rect reads index pel (i, y) -- two elements of index_format, or one complex element -- and gathers the input at
// it through EmbedFetch.  The fields the fetch reads are AffineArgs'.
struct MapimArgs {
	const unsigned char *in;
	const unsigned char *index;
	unsigned char *out;
	long long in_stride, index_stride, out_stride; // bytes
	int in_left, in_top, in_width, in_height;      // the input window, pels of the whole image; in_width == 0: no window
	int im_width, im_height;                       // the whole input image
	int out_width, out_height;                     // the rect: `index` and `out` point at its first pel
	int bands;                                     // elements a pel of the input
	int index_format;
	int index_wide; // every index pel lies on a multiple of its own size: one load a pel
	int window_offset;
	int extend;         // VipsHipExtend
	const void *tables; // BicubicTables, interp_device.h
	unsigned char ink[VIPS_HIP_AFFINE_MAX_PEL];  // the pel of what the coordinate stage rejects
	unsigned char fill[VIPS_HIP_AFFINE_MAX_PEL]; // the pel round the image under extend black / white / background
};
int mapim_run(const char *domain, MapimArgs a, int format, int interpolate);
// ... vips_mapim_region_minmax of a rect of the index in one launch: bounds[0 .. 3] = min x, min y, max x, max y over
// the pels without a NaN, after floor / ceil and the clip to [-1, VIPS_MAX_COORD] (both monotonic: the extremes are
// taken in the index's own type, block by block, and merged as integers).  bounds is device memory the kernel's host
// side initialises; a rect of nothing but NaN leaves min > max.
constexpr int MAPIM_MAX_COORD = 10000000; // VIPS_MAX_COORD's default
int mapim_bounds_run(const char *domain, const unsigned char *index, long long index_stride, int width, int height, int index_format,
	int *bounds);
// ... vips_xyz: pel (x, y) of a two-band uint image holds (x, y)
int xyz_run(const char *domain, unsigned char *out, long long out_stride, int width, int height);
// mapim_tile: 0 / 1 the pels / rows of a block's patch, 2 / 3 of a wave's, 4 the most blocks a bounds launch has,
// 5 the threads of a block of the bounds and xyz kernels, 6 the bytes of a group of the xyz kernel
int mapim_tile(int what);
// correlation.hip: vips_fastcor and vips_spcor on checked images of one format (ops_correlation.cpp checks everything): ONE
// launch writes the whole output, width x height pels of `bands` elements.  Output band b reads band b of an operand of
// `bands` bands and band 0 of an operand of one.  spcor: `table` holds bands * ref_w * ref_h doubles, band-major, the
// ref's (rp - rmean[b]) in raster order, and c1 the bands doubles of spcor.c:146-149; both device memory.
struct CorrelationArgs {
	const unsigned char *in, *ref;
	unsigned char *out;
	const double *table, *c1;
	long long in_stride, ref_stride, out_stride; // bytes
	int width, height;                           // of the image and of the output
	int in_bands, ref_bands, bands;
	int ref_w, ref_h;
};
int correlation_run(const char *domain, CorrelationArgs a, int format, int spcor);
// correlation_tile: 0 / 1 the pels / rows of a block's tile, 2 the largest ref side
int correlation_tile(int what);
// canvas.hip: vips_embed, vips_gravity, vips_insert and vips_join on checked geometry (ops_canvas.cpp checks everything):
// ONE launch writes the rect (out_left, out_top, out_width, out_height) of a canvas.  Canvas pel (X, Y) is the sub-image's
// pel where the sub-image lies, else the main image's pel where that lies, else -- by `mode` -- the ink, or the main
// image's pel at the clamped (copy), clock-arithmetic (repeat) or reflected (mirror) coordinate.  `main` points at pel
// (win_left, win_top) of the main image: the caller has checked that every pel the rect draws on lies in what it holds.
enum { CANVAS_INK = 0, CANVAS_COPY = 1, CANVAS_REPEAT = 2, CANVAS_MIRROR = 3 };
constexpr int CANVAS_MAX_PEL = 32; // bytes
struct CanvasArgs {
	const unsigned char *main;
	const unsigned char *sub; // nullptr: none
	unsigned char *out;       // pel (out_left, out_top) of the canvas
	long long main_stride, sub_stride, out_stride; // bytes
	int mx, my, mw, mh; // where the main image's pel (0, 0) lies on the canvas, its whole size
	int win_left, win_top;
	int sx, sy, sw, sh; // the sub-image
	int out_left, out_top, out_width, out_height;
	int pel;    // bytes
	int mode;   // CANVAS_*
	int groups; // (stream kernel) 16- / 48-byte groups of a row of the rect, the ragged one included
	unsigned int ink[CANVAS_MAX_PEL / 4];
};
int canvas_run(const char *domain, CanvasArgs a);
// canvas_tile: 0 the threads of a block, 1 the bytes of a group of the stream kernel for a pel size (0: the stream
// kernel does not take it), 2 the most blocks a launch has
int canvas_tile(int what, int pel);
// ... vips_flatten's generate functions (flatten.c:167-419): `format` uchar takes the table kernels, everything else the
// double macros; `black` the black-background path.  `ink` holds bands - 1 elements of `format`.
constexpr int FLATTEN_MAX_INK = 256; // bytes
struct FlattenArgs {
	const unsigned char *in;
	unsigned char *out;
	long long in_stride, out_stride; // bytes
	int width, height, bands;        // of the input
	int black;
	double max_alpha;
	unsigned long long ink[FLATTEN_MAX_INK / 8];
};
int flatten_run(const char *domain, FlattenArgs a, int format);
// ... vips_addalpha: every pel's `bands` elements of `es` bytes, then `alpha` (the low es bytes)
int addalpha_run(const char *domain, const unsigned char *in, long long in_stride, unsigned char *out, long long out_stride,
	int width, int height, int bands, int es, unsigned long long alpha);
// ops_canvas.cpp: vips__bandup (arithmetic.c:175-202) of a one-band image, the result tagged `interpretation`
int bandup(_VipsHipImage *in, _VipsHipImage **out, int n, int interpretation);
// cells.hip: vips_arrayjoin, vips_replicate, vips_wrap and vips_grid on checked geometry (ops_cells.cpp checks everything):
// ONE launch writes the rect (out_left, out_top, out_width, out_height) of an output that is a lattice of cells of
// cell_w x cell_h pels.  Output pel (X, Y) lies in cell (cx, cy) = ((X + org_x) / cell_w, (Y + org_y) / cell_h); a cell
// shows pels of one source row or the ink.  Which source:
//   CELLS_TABLE   descriptor min(n - 1, cx + cy * across) of `table` (arrayjoin.c:119,145): image pel (X - x0, Y - y0)
//                 where the image has one, else the ink
//   CELLS_REPEAT  the cell is one period of `src` (org_x, org_y in [0, sw] x [0, sh]: where the output's pel (0, 0) lies
//                 in its period): pel ((X + org_x) mod sw, (Y + org_y) mod sh)
//   CELLS_GRID    cell (cx, cy) is rows (cy * across + cx) * cell_h ... of `src` (grid.c:103,136)
// `src` points at pel (win_left, win_top) of the image of sw x sh pels.
enum { CELLS_TABLE = 0, CELLS_REPEAT = 1, CELLS_GRID = 2 };
struct CellDesc {
	const unsigned char *base; // the image's pel (0, 0)
	long long stride;          // bytes
	int x0, y0;                // where that pel lies on the output: negative steps into a cell where the image is cropped
	int w, h;                  // the image
};
struct CellsArgs {
	const CellDesc *table; // CELLS_TABLE: n descriptors in device memory
	const unsigned char *src;
	unsigned char *out; // pel (out_left, out_top) of the output
	long long src_stride, out_stride; // bytes
	int mode;                         // CELLS_*
	int n, across;
	int cell_w, cell_h, org_x, org_y;
	int sw, sh, win_left, win_top;
	int out_left, out_top, out_width, out_height;
	int pel;    // bytes
	int groups; // (stream kernel) 16- / 48-byte groups of a row of the rect, the ragged one included
	unsigned int ink[CANVAS_MAX_PEL / 4];
};
// `starts`: every source's base and stride or-ed together (what the row starts of all sources are multiples of)
int cells_run(const char *domain, CellsArgs a, unsigned long long starts);
// cells_tile: as canvas_tile
int cells_tile(int what, int pel);
// pointwise.h: the geometry of a pointwise launch on checked operands: ONE launch writes `height` rows of `elems` output
// elements.  Output element e of row y is made from element e of the operand's row, or -- an operand of one element a
// pel (b1 / b2 == 1) against `bands` -- from element e / bands; an operand is zero right of its w1 / w2 pels and below
// its h1 / h2 rows (vips__sizealike: embedded black at (0, 0)).
struct PointwiseGeom {
	const unsigned char *in;
	const unsigned char *in2; // the right-hand operand of the binary operations
	unsigned char *out;
	long long in_stride, in2_stride, out_stride; // bytes
	int elems, height;                            // of the output
	int bands;                                    // elements a pel of the output
	int w1, h1, b1, w2, h2, b2;
	int groups; // (stream kernel) 16-byte groups of an output row, the ragged one included
};
// ops_arith.cpp: the geometry of a unary call on a pair of windows, and of a binary call on two images and the output
void pointwise_unary_geom(const VipsHipRegion *in, const VipsHipRegion *out, PointwiseGeom *g);
void pointwise_binary_geom(const _VipsHipImage *left, const _VipsHipImage *right, const _VipsHipImage *out, PointwiseGeom *g);
// ... what a call on two images does between its null checks and its launch: the images are on one device, `plan`
// (vips_hip_binary_plan, vips_hip_logic_plan) fills the result's header, what is not in the common format is cast
// (vips__formatalike), the rows are short enough to index, the output is made and `geom` filled
struct BinaryOperands {
	int format, out_format, bands, interpretation, width, height;
	ImageRef cast[2], out;
	PointwiseGeom geom;
};
typedef int (*BinaryPlanFn)(const void *closure, const _VipsHipImage *left, const _VipsHipImage *right, BinaryOperands *b);
int binary_operands(const char *domain, _VipsHipImage *left, _VipsHipImage *right, BinaryPlanFn plan, const void *closure, BinaryOperands *b);
// arith.hip: the pointwise operations of arithmetic/ (ops_arith.cpp checks everything)
enum {
	ARITH_LINEAR = 0, ARITH_INVERT, ARITH_ABS, ARITH_ADD, ARITH_SUBTRACT, ARITH_MULTIPLY, ARITH_DIVIDE,
	ARITH_ROUND, ARITH_SIGN, ARITH_CLAMP, ARITH_MINPAIR, ARITH_MAXPAIR, ARITH_REMAINDER, ARITH_REMAINDER_CONST, ARITH_LAST
};
enum { ROUND_RINT = 0, ROUND_CEIL, ROUND_FLOOR, ROUND_LAST }; // VipsOperationRound
constexpr int ARITH_MAX_VECTOR = 32; // elements of vips_linear's a and b once they differ from band to band
// the operations with a right-hand image
constexpr bool arith_binary(int op)
{
	return (op >= ARITH_ADD && op <= ARITH_DIVIDE) || (op >= ARITH_MINPAIR && op <= ARITH_REMAINDER);
}
struct ArithArgs : PointwiseGeom {
	int single; // vips_linear: every element of a and of b the same (LOOP1, linear.c:213-223)
	float a1, b1f; // ... those, as the float the reference makes of them
	int round; // vips_round: ROUND_*
	// a_ready, b_ready (linear.c:181-200); vips_clamp: min in a[0], max in b[0]; vips_remainder_const: c_int in a
	double a[ARITH_MAX_VECTOR], b[ARITH_MAX_VECTOR];
};
int arith_run(const char *domain, int op, int in_format, int out_format, ArithArgs a);
// arith_tile: 0 the threads of a block, 1 the bytes of a group of the stream kernels, 2 / 3 the most blocks a pointwise /
// a statistics launch has
int arith_tile(int what);
// recomb.hip: vips_recomb (conversion/recomb.c) on checked geometry (ops_recomb.cpp checks everything): every pel's
// `mwidth` elements against the `mheight` rows of `matrix` (host memory, row-major), float out (double for double in)
constexpr int RECOMB_MAX = 32; // columns and rows of the matrix
constexpr int RECOMB_STREAM_MAX = 4; // ... of the shapes the stream kernel is compiled for
struct RecombArgs {
	const unsigned char *in;
	unsigned char *out;
	long long in_stride, out_stride; // bytes
	int width, height; // pels, rows
	int mwidth, mheight;
	int runs; // (stream kernel) runs of pels of a row, the ragged one included
	const double *matrix; // (general kernel) device memory
	double m[RECOMB_STREAM_MAX * RECOMB_STREAM_MAX]; // (stream kernel) the coefficients, row-major
};
int recomb_run(const char *domain, int format, RecombArgs a, const double *matrix);
// recomb_tile: 0 the threads of a block, 1 the most blocks of a stream launch, 2 the most pels of a stream kernel's run
int recomb_tile(int what);
// nary.hip: vips_sum (arithmetic/sum.c) and vips_bandrank (conversion/bandrank.c) over n images of one format on checked
// geometry (ops_nary.cpp checks everything): ONE launch, the images' base pointers and strides in the kernel's
// arguments.  Output element e of row y takes element e of every image's row, or -- an image of one band against
// `bands` -- element e / bands; an image is zero right of its width and below its height (vips__sizealike).
enum { NARY_SUM = 0, NARY_MIN, NARY_MAX, NARY_RANK, NARY_LAST }; // bandrank's index 0, n - 1 and any other
constexpr int NARY_IMAGES = 16;
struct NarySource {
	const unsigned char *in;
	long long stride; // bytes
	int width, height, bands, pad;
};
struct NaryArgs {
	unsigned char *out;
	long long out_stride; // bytes
	int elems, height, bands; // of the output
	int n, index; // images; NARY_RANK: the index-th smallest
	int groups; // (stream kernel) groups of an output row, the ragged one included
	NarySource src[NARY_IMAGES];
};
int nary_run(const char *domain, int op, int format, NaryArgs a);
// nary_tile: 0 the threads of a block, 1 the most blocks a launch has (a stream launch's blocks, the blocks_x * grid.y of
// a general one), 2 the bytes of the output a lane of the stream kernel makes at a time for sum and bandrank's minimum
// and maximum, 3 / 4 for bandrank's other indices on formats of up to four bytes / on double
int nary_tile(int what);
// ops_logic.cpp: vips__bandalike_vec (arithmetic.c:210-254) over n images
int bandalike(const char *domain, const int *bands, const int *interpretations, int n, int *out_bands, int *interpretation);
// ... vips_stats' scan (stats.c:247-330) of a whole image of uchar, char, ushort, short or float: every block's
// partial of every band goes to `slab` (blocks * bands entries, block-major), the host merges them in index order.
// Sums of integer images are 64-bit integers, of float images doubles (as bits); extremes carry the raster index
// y * width + x of their first pel, STATS_NONE for none (a band of nothing but NaN).
constexpr unsigned int STATS_NONE = 0xffffffffu;
struct StatsPartial {
	unsigned long long sum, sum2;
	unsigned int mn, mx;   // the value's bits (integers sign-extended to 32)
	unsigned int imn, imx;
};
// stats_blocks: how many blocks stats_run will launch for this image (the slab's size / bands)
int stats_blocks(const _VipsHipImage *in);
int stats_run(const char *domain, const _VipsHipImage *in, StatsPartial *slab);
// ops_arith.cpp: the common format of two (arithmetic.c:76-109), for every operation that runs vips__formatalike
int format_common(int a, int b);
// header_rules.cpp: the reference's header rules (iofuncs/header.c).  interpretation_bands: the "real" bands a tag
// implies, 0 for no idea; guess_interpretation: the tag, or the default for the format and the bands where the tag
// cannot be true of the image (a VipsInterpretation, which may be one vips_hip.h has no name for)
int interpretation_bands(int interpretation);
double interpretation_max_alpha(int interpretation);
int guess_interpretation(int interpretation, int width, int height, int bands, int format);
double format_max(int format); // -1 for the float formats
// ... VIPS_CLIP, and one element of vips__vector_to_pels: a constant as an element of `format` (real formats)
double vips_clip(double lo, double v, double hi);
void element_to_format(double real, int format, unsigned char *dst);
// ... vips_check_noncomplex's words for a complex format
int arithmetic_noncomplex(const char *domain, int format);
// ops_arith.cpp: a pair of windows of the same size, non-complex, not in place
int arithmetic_window_pair(const char *domain, const VipsHipRegion *in, const VipsHipRegion *out);
// logic.hip: the comparisons and booleans of arithmetic/relational.c and boolean.c (ops_logic.cpp checks everything).
// in2 == nullptr: the right-hand side is the constants (unaryconst.c:90-120).
enum { LOGIC_RELATIONAL = 0, LOGIC_BOOLEAN };
enum { RELATIONAL_EQUAL = 0, RELATIONAL_NOTEQ, RELATIONAL_LESS, RELATIONAL_LESSEQ, RELATIONAL_MORE, RELATIONAL_MOREEQ, RELATIONAL_LAST };
enum { BOOLEAN_AND = 0, BOOLEAN_OR, BOOLEAN_EOR, BOOLEAN_LSHIFT, BOOLEAN_RSHIFT, BOOLEAN_LAST };
constexpr int LOGIC_MAX_VECTOR = 32; // constants once they differ from band to band
struct LogicArgs : PointwiseGeom {
	int single; // every constant the same
	int is_int; // relational_const compares with c_int (relational.c:528-529)
	int c_int[LOGIC_MAX_VECTOR];
	double c_double[LOGIC_MAX_VECTOR];
};
int logic_run(const char *domain, int family, int op, int format, LogicArgs a);
// ... vips_ifthenelse (conversion/ifthenelse.c): `cond` uchar, of `bands` or of one element a pel; the then and else
// operands of one format, each of `bands` or of one element a pel; zero outside an operand's rectangle
struct SelectArgs {
	const unsigned char *cond, *in, *in2;
	unsigned char *out;
	long long cond_stride, in_stride, in2_stride, out_stride;
	int elems, height, bands;
	int wc, hc, bc, w1, h1, b1, w2, h2, b2;
	int groups; // (stream kernel) a lane's units of a row
};
int select_run(const char *domain, int format, int blend, SelectArgs a);
// ... the band operations: BAND_JOIN gathers every output pel from a table of sources -- source i gives the output's
// bands begin .. end - 1 from its elements first .. of each pel (bandjoin: first == 0 and all its bands; extract_band:
// one source); a source without a pointer gives `value`, a constant already in the image's format (bandjoin_const);
// a source is zero outside its rectangle.  BAND_MEAN, BAND_AND, BAND_OR, BAND_EOR fold all pel_elems elements of
// every pel of source 0 into one.
enum { BAND_JOIN = 0, BAND_MEAN, BAND_AND, BAND_OR, BAND_EOR };
constexpr int BAND_MAX_SOURCES = 16;
struct BandSource {
	const unsigned char *in;
	long long stride;
	unsigned long long value;
	int pel_elems, first, begin, end, width, height;
};
struct BandArgs {
	unsigned char *out;
	long long out_stride;
	int elems, height, out_bands; // of the output
	int n;
	int groups; // (stream kernel)
	BandSource src[BAND_MAX_SOURCES];
};
int band_run(const char *domain, int op, int format, BandArgs a);
// logic_tile: 0 the threads of a block, 1 the bytes of a group of the stream kernels, 2 the most blocks a stream launch has
int logic_tile(int what);
// trim.hip: vips_project's sums (project.c:221-298, combine sum) of a whole image in ONE launch.  Integer formats: the
// sums are ADDED to `columns` (width * bands) and `rows` (height * bands) 32-bit words, zero before the launch.  float
// and double: the blocks' partials go to col_part (grid[1] rows of width * bands doubles) and row_part (grid[0] rows of
// height * bands), project_grid() giving the grid; the block that takes the last ticket (*ticket zero before the launch)
// adds them in index order and writes both outputs.
void project_grid(const _VipsHipImage *in, int grid[3]);
int project_run(const char *domain, const _VipsHipImage *in, void *columns, void *rows, double *col_part, double *row_part,
	unsigned int *ticket);
// ... vips_profile's scan (profile.c:184-254): integer minima into `columns` (width * bands ints holding `height` before
// the launch) and `rows` (height * bands ints holding `width`)
int profile_run(const char *domain, const _VipsHipImage *in, int *columns, int *rows);
// ... vips_find_trim's scan of a uchar image of 1 .. 4 bands in ONE launch: the 3 x 3 median (`median`; else the pel
// itself), table[band * 256 + value] != 0 as the predicate of an element, and into bounds[0 .. 3] the maxima of
// width - x, x + 1, height - y, y + 1 over the pels with an element whose predicate holds (zero before the launch:
// zero after it says no pel is set).  `table` (256 * bands bytes) and `bounds` are device memory.
int trim_fused_run(const char *domain, const _VipsHipImage *in, int median, const unsigned char *table, unsigned int *bounds);
// trim_tile: 0 the threads of a block, 1 the bytes of a group of project_stream, 2 the rows of a fused tile, 3 the most
// blocks a project / profile launch has once more than one row of blocks is needed, 4 the elements of a fused tile's row,
// 5 the rows a fused block takes, 6 the rows between two meetings of a project / profile block's waves
int trim_tile(int what);
// regions.hip: vips_labelregions of a checked image (ops_regions.cpp checks everything) in six launches.  `planes` is
// device memory of regions_layout()'s `bytes`: the parent plane (width * height ints), the seams' bits, the chunk counts
// and the total, at the offsets the layout gives; all of it is rewritten by every call.  `out` is the mask, width *
// height ints.  After the run the int at planes + layout.total holds the number of regions.
constexpr int REGIONS_MAX_PEL = 32; // bytes
struct RegionsLayout {
	size_t parent, vseam, hseam, counts, total; // offsets into the planes, bytes
	size_t bytes;
	long long n_vseam, n_hseam; // seam bytes: (tiles across - 1) * height, (tiles down - 1) * width
	int chunks;
};
void regions_layout(int width, int height, RegionsLayout *l);
int regions_label_run(const char *domain, const _VipsHipImage *in, unsigned char *planes, int *out);
// ... vips_countlines' count in ONE read-only launch: the rises (an element below 128 followed by one at or above it,
// down the columns, or along the rows for `vertical`) of every band are ADDED to *rises, device memory, zero before
int countlines_run(const char *domain, const _VipsHipImage *in, int vertical, unsigned long long *rises);
// regions_tile: 0 / 1 the pels / rows of a tile of label_tiles, 2 the largest pel in bytes, 3 the linear indices of a chunk
int regions_tile(int what);
} // namespace vh
