/* vips_hip.h -- C ABI of libvipship.so: the MI355X (gfx950) implementation of
 * libvips' per-tile pixel pipeline (resample/, convolution/, colour/ hot loops).
 *
 * This header is the drop-in boundary.  Everything is plain C: pointers, ints,
 * doubles and two POD structs.  No HIP, torch or glib type appears in a
 * signature, so the libvips side (a C module registering `*_hip` VipsOperation
 * classes, see host/ and INTEGRATION.md) and any FFI (ctypes, cgo, JNI...) can
 * bind it directly.
 *
 * Three layers, mirroring the reference (all paths relative to the reference
 * tree, libvips 8.19.0):
 *
 *   1. runtime      device / stream / memory / error buffer
 *                   (error convention of iofuncs/error.c: 0 or -1 + message)
 *   2. region ops   "generate" replacements: fill out->valid from an input
 *                   region, exactly the contract of VipsGenerateFn
 *                   (include/vips/image.h:151-154, iofuncs/region.c:1600-1624)
 *   3. image ops    whole-image operations on device-resident images, the
 *                   analogue of the vips_reduce()/vips_conv()/... C wrappers;
 *                   they do what each class's build() does on the host (sizes,
 *                   tables, embed offsets) and then run the region ops once
 *                   over the whole output.
 *
 * Pixel layout everywhere: interleaved bands, row-major, `stride` bytes per line
 * (include/vips/image.h:382-393, include/vips/region.h:198-236).
 */
#ifndef VIPS_HIP_H
#define VIPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIPS_HIP_API __attribute__((visibility("default")))

/* Same values as VipsBandFormat, include/vips/image.h:120-133. */
typedef enum {
	VIPS_HIP_FORMAT_UCHAR = 0,
	VIPS_HIP_FORMAT_CHAR = 1,
	VIPS_HIP_FORMAT_USHORT = 2,
	VIPS_HIP_FORMAT_SHORT = 3,
	VIPS_HIP_FORMAT_UINT = 4,
	VIPS_HIP_FORMAT_INT = 5,
	VIPS_HIP_FORMAT_FLOAT = 6,
	VIPS_HIP_FORMAT_COMPLEX = 7,
	VIPS_HIP_FORMAT_DOUBLE = 8,
	VIPS_HIP_FORMAT_DPCOMPLEX = 9
} VipsHipFormat;

/* Same values as VipsKernel, include/vips/resample.h:41-51. */
typedef enum {
	VIPS_HIP_KERNEL_NEAREST = 0,
	VIPS_HIP_KERNEL_LINEAR = 1,
	VIPS_HIP_KERNEL_CUBIC = 2,
	VIPS_HIP_KERNEL_MITCHELL = 3,
	VIPS_HIP_KERNEL_LANCZOS2 = 4,
	VIPS_HIP_KERNEL_LANCZOS3 = 5,
	VIPS_HIP_KERNEL_MKS2013 = 6,
	VIPS_HIP_KERNEL_MKS2021 = 7
} VipsHipKernel;

/* The interpolators vips_resize picks for upsizing (resample/resize.c:118-133). */
typedef enum {
	VIPS_HIP_INTERPOLATE_NEAREST = 0,
	VIPS_HIP_INTERPOLATE_BILINEAR = 1,
	VIPS_HIP_INTERPOLATE_BICUBIC = 2
} VipsHipInterpolate;

/* Same values as VipsPrecision, include/vips/basic.h:106-110. */
typedef enum {
	VIPS_HIP_PRECISION_INTEGER = 0,
	VIPS_HIP_PRECISION_FLOAT = 1,
	VIPS_HIP_PRECISION_APPROXIMATE = 2
} VipsHipPrecision;

/* The subset of VipsInterpretation (include/vips/image.h:94-118) the colour
 * path routes between, and HISTOGRAM, which vips_hip_hist_find's result carries; same values.
 */
typedef enum {
	VIPS_HIP_INTERPRETATION_MULTIBAND = 0,
	VIPS_HIP_INTERPRETATION_B_W = 1,
	VIPS_HIP_INTERPRETATION_HISTOGRAM = 10,
	VIPS_HIP_INTERPRETATION_XYZ = 12,
	VIPS_HIP_INTERPRETATION_LAB = 13,
	VIPS_HIP_INTERPRETATION_LABS = 21,
	VIPS_HIP_INTERPRETATION_sRGB = 22,
	VIPS_HIP_INTERPRETATION_RGB16 = 25,
	VIPS_HIP_INTERPRETATION_GREY16 = 26,
	VIPS_HIP_INTERPRETATION_scRGB = 28
} VipsHipInterpretation;

/* ------------------------------------------------------------------ runtime */

/* Bind the CALLING THREAD to a device (hipSetDevice is per thread) and create the library's
 * per-device state on it: the HBM pool, the plan caches and the thread's stream are per device,
 * so one process can drive every GPU of a node from its threads -- the shape of libvips' own
 * parallelism, a worker pool inside one process (iofuncs/threadpool.c:625) -- as well as the
 * one-process-per-GPU shape of the multi-rank programs.  Safe to call repeatedly; calling it
 * with another device re-binds the thread (its external stream, if any, is dropped).
 *
 * A thread that never calls it is bound on first use: to the next entry of $VIPS_HIP_DEVICES (a
 * comma list, e.g. "0,1,2,3,4,5,6,7", dealt round-robin over such threads -- how the libvips
 * module spreads a worker pool over the GPUs), else to $VIPS_HIP_DEVICE, else to the device of
 * the process's first vips_hip_init(), else to device 0.
 *
 * Library-made images remember their device and every image-level operation runs on the device
 * its input lives on (the calling thread is re-bound if need be); plan handles
 * (vips_hip_reduce_new() ...) belong to the device of the thread that made them and fail loudly
 * on another.  Fails (-1) when no gfx950 device is visible: there is NO CPU fallback anywhere in
 * this library.
 */
VIPS_HIP_API int vips_hip_init(int device);
/* Finish and drop the calling thread's streams and cached blocks; the thread may bind again. */
VIPS_HIP_API void vips_hip_shutdown(void);
VIPS_HIP_API int vips_hip_device_count(void);
/* The device the calling thread is bound to, -1 when it has not been bound yet. */
VIPS_HIP_API int vips_hip_current_device(void);
/* The devices work is spread over: $VIPS_HIP_DEVICES in order (entries may repeat), else the
 * calling thread's device alone.  Fills devices[0 .. max) and returns how many there are,
 * -1 on a malformed list.
 */
VIPS_HIP_API int vips_hip_devices(int *devices, int max);

/* Thread-local error log, same shape as vips_error_buffer()/vips_error_clear()
 * (iofuncs/error.c): messages are "domain: text\n".
 */
VIPS_HIP_API const char *vips_hip_error_buffer(void);
VIPS_HIP_API void vips_hip_error_clear(void);

/* The stream all following calls of this thread are enqueued on.  NULL selects
 * the library's own per-thread stream (one per libvips worker thread, created in
 * start_fn and released in stop_fn by the module).  The handle is a hipStream_t
 * passed as void*, e.g. torch.cuda.current_stream().cuda_stream.
 */
VIPS_HIP_API int vips_hip_set_stream(void *stream);
VIPS_HIP_API void *vips_hip_get_stream(void);
VIPS_HIP_API int vips_hip_synchronize(void);
/* vips_vector_set_enabled / vips_vector_isenabled (iofuncs/vector.cpp:98-113).  A Highway-built
 * libvips computes convi on uchar images with 8-bit mantissas and a shared exponent
 * (convolution/convi.c:925-1120, convi_hwy.cpp) whenever vectors are enabled and the mask fits;
 * its other vector paths equal the C paths bit for bit.  Enabling this makes vips_hip_conv /
 * convsep / gaussblur with precision INTEGER on uchar compute exactly that, so that this
 * library can stand in for such a build.  Default: disabled (the C path's arithmetic).
 */
VIPS_HIP_API void vips_hip_vector_set_enabled(int enabled);
VIPS_HIP_API int vips_hip_vector_isenabled(void);

/* Float arithmetic mode.  The reference is baseline x86-64 C: a double sum is a chain of
 * separately rounded multiplies and adds (convolution/convf.c:163-181).  By default the large
 * float convolutions on integer images (masks 8 or more wide: BASELINE config 5) accumulate
 * with fused multiply-adds instead -- twice the FP64 rate, and the float result differs from the
 * reference's by at most 1 ULP where the taps are of one sign and the pels under a window are of
 * one sign, so that the sum cannot cancel (the tolerance BASELINE.json's north_star grants float
 * paths; measured: a handful of pixels per million).  A window that holds pels of both signs can
 * cancel, and what is left of a cancelled sum has no ULP bound in either arithmetic.  Masks
 * whose non-zero taps differ in sign always take the exact arithmetic, whatever the mode; so do
 * the operations a decision hangs on (vips_hip_canny, vips_hip_smartcrop's attention search)
 * while they run.  Enabled (or $VIPS_HIP_EXACT_FLOAT=1 at first use) every float path reproduces
 * the reference bit for bit.  Integer paths are always exact.
 */
VIPS_HIP_API void vips_hip_set_exact_float(int enabled);
VIPS_HIP_API int vips_hip_get_exact_float(void);

/* Device memory comes from a size-bucketed caching pool (hipMalloc is far too
 * slow to sit in a per-tile path); *_host is pinned staging memory.
 */
VIPS_HIP_API void *vips_hip_malloc(size_t size);
VIPS_HIP_API void vips_hip_free(void *ptr);
VIPS_HIP_API void *vips_hip_malloc_host(size_t size);
VIPS_HIP_API void vips_hip_free_host(void *ptr);
VIPS_HIP_API int vips_hip_memcpy_h2d(void *dst, const void *src, size_t size);
VIPS_HIP_API int vips_hip_memcpy_d2h(void *dst, const void *src, size_t size);
VIPS_HIP_API int vips_hip_memcpy_d2d(void *dst, const void *src, size_t size);
/* The same copies QUEUED on the calling thread's current stream (pinned host memory --
 * vips_hip_malloc_host() -- for them to overlap anything): how the module's strip loop keeps
 * the upload of strip k + 1, the kernels of strip k and the download of strip k - 1 in flight
 * together, the way sinkdisc.c:177-220 writes one buffer behind the one being filled.
 */
VIPS_HIP_API int vips_hip_memcpy_h2d_async(void *dst, const void *src, size_t size);
VIPS_HIP_API int vips_hip_memcpy_d2h_async(void *dst, const void *src, size_t size);
/* A stream of the calling thread's device, for vips_hip_set_stream(); freed after a
 * synchronize. */
VIPS_HIP_API void *vips_hip_stream_new(void);
VIPS_HIP_API void vips_hip_stream_free(void *stream);
VIPS_HIP_API int vips_hip_memcpy2d_h2d(void *dst, size_t dpitch,
	const void *src, size_t spitch, size_t width_bytes, size_t height);
VIPS_HIP_API int vips_hip_memcpy2d_d2h(void *dst, size_t dpitch,
	const void *src, size_t spitch, size_t width_bytes, size_t height);
VIPS_HIP_API size_t vips_hip_pool_bytes(void);
VIPS_HIP_API void vips_hip_pool_trim(void);

/* HIP events on the current stream, for timing kernels where they run. */
VIPS_HIP_API void *vips_hip_event_new(void);
VIPS_HIP_API void vips_hip_event_free(void *event);
VIPS_HIP_API int vips_hip_event_record(void *event);
VIPS_HIP_API double vips_hip_event_elapsed_ms(void *start, void *stop); /* syncs on stop */
VIPS_HIP_API int vips_hip_event_synchronize(void *event); /* wait on the host for a recorded event */
VIPS_HIP_API int vips_hip_stream_wait_event(void *event); /* the current stream waits for it */

/* Per-kernel timing (the VIPS_GATE_START/STOP analogue, include/vips/gate.h):
 * when enabled every kernel launch is bracketed by events on its stream.
 */
VIPS_HIP_API void vips_hip_gate_enable(int enable);
VIPS_HIP_API void vips_hip_gate_reset(void);
/* Returns the number of launches of kernels whose gate name starts with @name
 * and their total duration in ms (synchronises the device).
 */
VIPS_HIP_API int vips_hip_gate_query(const char *name, double *total_ms);
/* Write "name launches total_ms\n" for every gate name seen into @buf (at most
 * @size bytes, NUL-terminated); returns the number of distinct names.
 */
VIPS_HIP_API int vips_hip_gate_report(char *buf, int size);

/* ---------------------------------------------------------------- regions */

/* A window onto a device-resident image: the VipsRegion of this library
 * (include/vips/region.h:96-131).  `data` points at pixel (left, top) of the
 * full image; `stride` is VIPS_REGION_LSKIP.  im_width/im_height are the
 * size of the whole image the window belongs to: coordinates that an operation
 * computes outside [0, im_width) x [0, im_height) are clamped to the edge, which
 * is what the vips_embed(VIPS_EXTEND_COPY) each reference build() inserts does
 * (conversion/embed.c:226-341).  After clamping they must fall inside the window.
 */
typedef struct {
	void *data;
	int left, top, width, height; /* valid: the window */
	int im_width, im_height;      /* the whole image */
	int bands;
	int format; /* VipsHipFormat */
	size_t stride;
} VipsHipRegion;

/* ------------------------------------------------ resample: reduceh/reducev */

/* Host-side state of one reduceh/reducev operation: what vips_reduceh_build()
 * (resample/reduceh.cpp:396-565) / vips_reducev_build() (reducev.cpp:859-1075)
 * compute once per call -- output size, n_point, h/v offset, the 65 x n_point
 * coefficient tables matrixf (double) and matrixs (short, x4096, truncated) --
 * kept resident on the device.
 */
typedef struct _VipsHipReduce VipsHipReduce;

/* @in_size: Xsize (horizontal) or Ysize (vertical) of the input image.
 * @shrink:  the *residual* shrink (after any integer pre-shrink the caller did).
 * @extra_pixels: "how many pixels we are inventing", already divided by the
 *   integer pre-shrink (reduceh.cpp:431,459); pass NAN to have it derived as
 *   out_size * shrink - in_size.
 * Errors (message as the reference's): "reduce factor should be >= 1.0",
 * "reduce factor too large", "image has shrunk to nothing".
 */
VIPS_HIP_API VipsHipReduce *vips_hip_reduce_new(int kernel, double shrink,
	int in_size, int out_size, double extra_pixels);
VIPS_HIP_API void vips_hip_reduce_free(VipsHipReduce *reduce);
VIPS_HIP_API int vips_hip_reduce_get_n_point(const VipsHipReduce *reduce);
VIPS_HIP_API int vips_hip_reduce_get_out_size(const VipsHipReduce *reduce);
VIPS_HIP_API double vips_hip_reduce_get_offset(const VipsHipReduce *reduce);
/* Copy out row @phase (0..64) of matrixs / matrixf, for tests. */
VIPS_HIP_API int vips_hip_reduce_get_matrixs(const VipsHipReduce *reduce, int phase, short *out);
VIPS_HIP_API int vips_hip_reduce_get_matrixf(const VipsHipReduce *reduce, int phase, double *out);

/* vips_reduce_get_points(), resample/reduceh.cpp:113-141. */
VIPS_HIP_API int vips_hip_reduce_get_points(int kernel, double shrink);

/* The input rectangle a generate needs for output rect (left, top, width,
 * height): reduceh.cpp:237-240 / reducev.cpp:539-542, already translated from
 * embedded to un-embedded input coordinates and clipped to the input image.
 */
VIPS_HIP_API void vips_hip_reduceh_need(const VipsHipReduce *reduce,
	int left, int width, int *in_left, int *in_width);
VIPS_HIP_API void vips_hip_reducev_need(const VipsHipReduce *reduce,
	int top, int height, int *in_top, int *in_height);

/* Fill out->valid.  Bit-exact replacements for vips_reduceh_gen
 * (reduceh.cpp:216-335) and vips_reducev_gen (reducev.cpp:517-619): the double
 * position accumulator is seeded at out->left / out->top exactly as the
 * reference seeds it per generate call.
 */
VIPS_HIP_API int vips_hip_reduceh_gen(const VipsHipReduce *reduce,
	const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_reducev_gen(const VipsHipReduce *reduce,
	const VipsHipRegion *in, const VipsHipRegion *out);
/* As above, but the accumulator is re-seeded every @tile rows (columns), which
 * reproduces what the reference computes when its sink walks the output in
 * @tile-high strips (thread.c:301-325: 16 for FATSTRIP images).  tile <= 0
 * means one seed for the whole rect.
 */
VIPS_HIP_API int vips_hip_reduceh_gen_tiled(const VipsHipReduce *reduce,
	const VipsHipRegion *in, const VipsHipRegion *out, int tile);
VIPS_HIP_API int vips_hip_reducev_gen_tiled(const VipsHipReduce *reduce,
	const VipsHipRegion *in, const VipsHipRegion *out, int tile);

/* Fused reducev -> reduceh for uchar images (the vips_reduce() hot path,
 * resample/reduce.c:98-121): the vertically reduced scanlines never leave the
 * CU.  Same results as running the two gens back to back.
 */
VIPS_HIP_API int vips_hip_reduce_gen(const VipsHipReduce *reducev,
	const VipsHipReduce *reduceh,
	const VipsHipRegion *in, const VipsHipRegion *out);
/* The vertical accumulator re-seeded every @tile output rows, as above.
 * Both return 0 on success, -1 on error, and 1 when the geometry (format,
 * bands, shrink) is outside what the fused kernel covers: nothing was written
 * and the caller runs vips_hip_reducev_gen + vips_hip_reduceh_gen instead.
 */
VIPS_HIP_API int vips_hip_reduce_gen_tiled(const VipsHipReduce *reducev,
	const VipsHipReduce *reduceh,
	const VipsHipRegion *in, const VipsHipRegion *out, int tile);

/* ------------------------------------------------- resample: shrinkh/shrinkv */

/* vips_shrinkh_gen / vips_shrinkv_gen (resample/shrinkh.c:235-283,
 * shrinkv.c:318-387).  Input coordinates beyond the image edge are clamped
 * (the reference embeds, shrinkh.c:383-386, shrinkv.c:501-506).
 */
VIPS_HIP_API int vips_hip_shrinkh_gen(int hshrink,
	const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_shrinkv_gen(int vshrink,
	const VipsHipRegion *in, const VipsHipRegion *out);
/* Output sizes: shrinkh.c:414-416, shrinkv.c:566-568. */
VIPS_HIP_API int vips_hip_shrink_out_size(int in_size, int shrink, int ceil_mode);

/* ------------------------------------------------------------------ upsizing */

/* vips_affine_gen (resample/affine.c:230-397) for the pure scale vips_resize asks for
 * (resize.c:268-300: matrix (hscale, 0, 0, vscale), "idx"/"idy" displacements, EXTEND_COPY,
 * premultiplied) with vips_interpolate_nearest / _bilinear (resample/interpolate.c:336-352,
 * 432-484) or _bicubic (resample/bicubic.cpp:482-600): fills @out's rect of the
 * vips_hip_affine_out_size() image from @in, whose window must hold the stencils.  The
 * reference accumulates a row's x coordinate from the first pixel of each generate rect;
 * @tile_width says where those rects start (multiples of it; 0 = whole rows, the FATSTRIP
 * geometry a scale-only affine requests, affine.c:575-579).  uchar ... int and float
 * (complex as float pairs); double images are refused (no-table bicubic).
 */
VIPS_HIP_API int vips_hip_upsize_gen(const VipsHipRegion *in, const VipsHipRegion *out,
	double hscale, double vscale, double idx, double idy, int interpolate, int tile_width);
/* Output size of the affine: VIPS_ROUND_INT(scale * in_size), resample/transform.c:220-231. */
VIPS_HIP_API int vips_hip_affine_out_size(int in_size, double scale);
/* vips_zoom (conversion/zoom.c): integral pixel replication, what vips_resize uses for
 * kernel nearest with integral scales (resize.c:257-266). */
VIPS_HIP_API int vips_hip_zoom_gen(const VipsHipRegion *in, const VipsHipRegion *out, int xfac, int yfac);
/* vips_subsample (conversion/subsample.c:148-240): out(x, y) = in(x * xfac, y * yfac), output
 * size in / fac; what vips_resize uses for the integer part of a nearest-neighbour shrink
 * (resize.c:165-203). */
VIPS_HIP_API int vips_hip_subsample_gen(const VipsHipRegion *in, const VipsHipRegion *out, int xfac, int yfac);
/* 0: the threads of a block of the upsize, zoom and subsample kernels (a pel a lane); 1: the most blocks a launch has
 * (the blocks of a row times the rows in flight; the other rows are taken in turns) -- for tests that want sizes
 * round them. */
VIPS_HIP_API int vips_hip_upsize_step(int what);

/* -------------------------------------------------------------- convolution */

/* Host-side state of one convi/convf: vips_convi_build (convolution/convi.c:
 * 1123-1233, C path) / vips_convf_build (convf.c:285-369): coefficients with
 * zeros squeezed out, their mask positions, scale/offset.
 */
typedef struct _VipsHipConv VipsHipConv;

/* @mask: mask_width x mask_height doubles, row-major (a VIPS matrix image).
 * precision INTEGER = convi C path, FLOAT = convf.
 */
VIPS_HIP_API VipsHipConv *vips_hip_conv_new(const double *mask,
	int mask_width, int mask_height, double scale, double offset, int precision);
VIPS_HIP_API void vips_hip_conv_free(VipsHipConv *conv);
VIPS_HIP_API int vips_hip_conv_get_nnz(const VipsHipConv *conv);
/* The Highway-variant view of an INTEGER plan (vips_convi_intize, convi.c:925-1120): the shared
 * exponent and the non-zero 8-bit mantissas with their mask positions.  Returns their number,
 * 0 when the intize refuses the mask (the C path runs even with vectors enabled), -1 on error. */
VIPS_HIP_API int vips_hip_conv_get_vector(const VipsHipConv *conv, int *exp, int *mant, int *pos, int max);
/* Output band format for input @format: convf.c:354-355; convi keeps it. */
VIPS_HIP_API int vips_hip_conv_out_format(const VipsHipConv *conv, int format);
/* Fill out->valid: vips_convi_gen (convi.c:753-857) or vips_convf_gen
 * (convf.c:185-283).  The input is the UN-embedded image; edge clamp included.
 */
VIPS_HIP_API int vips_hip_conv_gen(const VipsHipConv *conv,
	const VipsHipRegion *in, const VipsHipRegion *out);
/* 0: the threads of a block of the convolution kernels; 1: the most rows the one-element-a-lane kernel has in flight
 * (its blocks take the other rows in turns); 2: the most rows of blocks the register-tiled, grouped and row-streaming
 * kernels launch: taller outputs go to the one-element-a-lane kernel -- for tests that want sizes round them. */
VIPS_HIP_API int vips_hip_conv_step(int what);

/* precision=approximate.  Host-side state of one vips_conva (convolution/conva.c:676-767: the
 * rint()ed mask cut into `layers` slabs, every slab row a run of ones, near-identical runs
 * clustered within `cluster`, runs on consecutive rows joined into boxes) or one vips_convasep
 * (convolution/convasep.c:152-330, the 1-D form).  The decomposition fixes the approximated mask,
 * the divisor and the rounding term, so it has to be the reference's, quirk for quirk.
 */
typedef struct _VipsHipConva VipsHipConva;

VIPS_HIP_API VipsHipConva *vips_hip_conva_new(const double *mask,
	int mask_width, int mask_height, double scale, double offset, int layers, int cluster);
VIPS_HIP_API VipsHipConva *vips_hip_convasep_new(const double *mask,
	int mask_n, double scale, double offset, int layers);
VIPS_HIP_API void vips_hip_conva_free(VipsHipConva *plan);
/* The decomposition, for inspection (host only, no device needed).
 *   conva:    info = {n_runs, n_columns, divisor, rounding, offset, longest run};
 *             lines = n_runs x {start, end} then n_columns x {run, factor, first row, last row + 1}
 *             (the hlines and vlines of conva.c:140-205)
 *   convasep: info = {n_lines, divisor, rounding, offset, 0, 0}; lines = n x {start, end, factor}
 * Returns the number of ints written to @lines, or -1.
 */
VIPS_HIP_API int vips_hip_conva_get_lines(const VipsHipConva *plan, int *info, int *lines, int max_ints);
/* Fill out->valid: vips_conva_hgenerate + vips_conva_vgenerate (conva.c:876-1020, 1099-1198) in
 * one pass over the UN-embedded image; output format == input format.
 */
VIPS_HIP_API int vips_hip_conva_gen(const VipsHipConva *plan,
	const VipsHipRegion *in, const VipsHipRegion *out);
/* One pass of vips_convasep: vips_convasep_generate_horizontal (convasep.c:516-590, no offset) or
 * _vertical (:677-750, adds the offset).
 */
VIPS_HIP_API int vips_hip_convasep_gen(const VipsHipConva *plan,
	const VipsHipRegion *in, const VipsHipRegion *out, int vertical);
/* 0: the threads of a block of the approximate convolutions' kernels; 1: the most rows a launch has in flight (its
 * blocks take the other rows in turns). */
VIPS_HIP_API int vips_hip_conva_step(int what);

/* vips_gaussmat (create/gaussmat.c:95-167).  Writes at most @max doubles,
 * returns the mask width (height is 1 when separable, else == width), or -1.
 */
VIPS_HIP_API int vips_hip_gaussmat(double sigma, double min_ampl, int separable,
	int precision, double *mask, int max, double *scale);

/* ------------------------------------------------------------------- colour */

/* The per-scanline process_line functions (colour/colour.c:119-156), one call
 * per region.  in/out bands: 3 colour bands, any extra bands are copied through
 * with the format cast vips_colour_build does (colour.c:196-296).
 */
typedef enum {
	VIPS_HIP_COLOUR_sRGB2scRGB = 0, /* colour/sRGB2scRGB.c:72-106, uchar/ushort in, float out */
	VIPS_HIP_COLOUR_scRGB2XYZ,      /* scRGB2XYZ.c:58-82 */
	VIPS_HIP_COLOUR_XYZ2Lab,        /* XYZ2Lab.c:144-171 */
	VIPS_HIP_COLOUR_Lab2XYZ,        /* Lab2XYZ.c:114-143 */
	VIPS_HIP_COLOUR_XYZ2scRGB,      /* XYZ2scRGB.c:72-94 */
	VIPS_HIP_COLOUR_scRGB2sRGB,     /* scRGB2sRGB.c:84-132, float in, uchar out */
	VIPS_HIP_COLOUR_scRGB2sRGB16,   /* scRGB2sRGB.c, depth 16, ushort out */
	VIPS_HIP_COLOUR_Lab2LabS,       /* Lab2LabS.c:59-73 */
	VIPS_HIP_COLOUR_LabS2Lab,       /* LabS2Lab.c:55-69 */
	VIPS_HIP_COLOUR_sRGB2scRGB16,   /* sRGB2scRGB.c:91-105, RGB16 (ushort) in */
	/* greyscale and 16-bit RGB: the band count or the band format of the WHOLE pel changes */
	VIPS_HIP_COLOUR_scRGB2BW,       /* scRGB2BW.c:59-105 depth 8: float x 3 in, uchar x 1 out */
	VIPS_HIP_COLOUR_scRGB2BW16,     /* scRGB2BW.c, depth 16: ushort x 1 out */
	VIPS_HIP_COLOUR_BW2sRGB,        /* colourspace.c:152-175: the band three times, any format */
	VIPS_HIP_COLOUR_GREY162RGB16,   /* colourspace.c:177-186: the same, tagged RGB16 */
	VIPS_HIP_COLOUR_sRGB2RGB16,     /* colourspace.c:99-109: shift cast of every band to ushort */
	VIPS_HIP_COLOUR_RGB162sRGB,     /* colourspace.c:83-97: shift cast of every band to uchar */
	VIPS_HIP_COLOUR_LAST
} VipsHipColourStep;

VIPS_HIP_API int vips_hip_colour_gen(int step,
	const VipsHipRegion *in, const VipsHipRegion *out);
/* A whole colourspace route (colourspace.c:223-520) in one pass: the steps are
 * evaluated per pixel in registers with the reference's intermediate types, so the
 * result is bit-identical to running them as separate images.  Decoding steps
 * (sRGB2scRGB*, LabS2Lab) may only come first and encoding steps (scRGB2sRGB*,
 * Lab2LabS) only last.  The stored input may be uchar, ushort, short or float: it is
 * vips_cast to what the first step wants (colour.c:343-348,428-434).  @alpha_scale is
 * max_alpha_after / max_alpha_before for the extra bands (colour.c:257-273).
 * BW2sRGB / GREY162RGB16 may only come first (the input then has 1 colour band) and
 * scRGB2BW* only last (the output then has 1); the two shift casts stand alone or
 * straight behind a band-replicating step, act on every band and take no @alpha_scale.
 * The extra bands are in->bands minus the input's colour bands, and as many in @out.
 */
VIPS_HIP_API int vips_hip_colour_route_gen(const int *steps, int n_steps, double alpha_scale,
	const VipsHipRegion *in, const VipsHipRegion *out);

/* vips_cast (conversion/cast.c:120-330): clip + truncate between any two
 * non-complex band formats.
 */
VIPS_HIP_API int vips_hip_cast_gen(const VipsHipRegion *in, const VipsHipRegion *out);

/* vips_premultiply_gen (conversion/premultiply.c:134-214) / vips_unpremultiply_gen
 * (conversion/unpremultiply.c:198-262); the last band is alpha.  @uchar selects the
 * uchar -> uchar fixed-point fast path (scale table, (in * scale + 128) >> 8) that
 * vips_thumbnail uses (resample/thumbnail.c:848-904); otherwise the output is float.
 */
VIPS_HIP_API int vips_hip_premultiply_gen(const VipsHipRegion *in, const VipsHipRegion *out,
	double max_alpha, int uchar, int inverse);

/* vips_rot (conversion/rot.c) and vips_flip (conversion/flip.c): exact copies of pels, any band count and
 * format.  @angle is a VipsAngle (0 d0, 1 d90, 2 d180, 3 d270: d90 is a quarter turn clockwise, out(x, y) =
 * in(y, H-1-x)), @direction a VipsDirection (0 horizontal, 1 vertical).  @in's width x height pels at its data go
 * to @out's, which must have the turned size and the same bands and format; strides are free (a window of a larger
 * image on either side), left / top are not looked at.  Quarter turns run in a transposing tile kernel for pels of
 * 1, 2, 3, 4, 6, 8, 12 and 16 bytes (vips_hip_rot_tile_side: its tile side for a pel size, 0 for others), the
 * other operations in a streaming kernel where rows start on dwords; a one-pel-a-lane kernel takes the rest.
 */
VIPS_HIP_API int vips_hip_rot_gen(int angle, const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_flip_gen(int direction, const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_rot_tile_side(int pel_size);
/* 0: the threads of a block of the streaming and the one-pel-a-lane kernel; 1: the most blocks a launch of either has
 * (the blocks of a row times the rows in flight; the other rows are taken in turns) -- for tests that want sizes round
 * them. */
VIPS_HIP_API int vips_hip_rot_step(int what);
/* The bytes a lane of the streaming kernel takes at a time for @pel_size: 48 for a mirror of pels that do not divide
 * 16, else 16 (a row-permuted copy moves rows of bytes: pel size 1); 0 for pel sizes the kernel is not compiled for. */
VIPS_HIP_API int vips_hip_rot_group(int pel_size);

/* ----------------------------------------------------------------- morphology
 *
 * vips_rank_generate (morphology/rank.c:412-456): out element (x, y, b) is the @index-th smallest (from 0) of the
 * @width x @height window whose top-left is input pel (x - width / 2, y - height / 2), band b, pel coordinates clamped
 * to the image (the embed of rank.c:507-511).  uchar, char, ushort, short, uint, int and float; the output has the
 * input's format.  Errors with the reference's words: "window too large" (width > im_width or height > im_height),
 * "index out of range".  double images are refused.  Float results are defined for inputs without NaN (the
 * reference's own answer depends on which of its four routes runs) and compare equal by value: -0 sorts below +0.
 * Three kernels: rank_median3 (3 x 3, index 4), rank_minmax (index 0 or n - 1, separable), rank_select (the rest:
 * bisection on an order-preserving key).  The window is limited by the kernels' LDS only: 8 + height - 1 staged rows
 * of 256 + (width - 1) * bands elements -- and as many rows of 256 more for rank_minmax -- must fit a CU's 160 KB;
 * 31 x 31 fits for every format up to 16 bands, what does not fit is refused with the sizes in the message.
 *
 * vips_erode_gen / vips_dilate_gen (morph.c:662-826): @mask is mask_width x mask_height doubles of 0, 128 and 255
 * (after rint(); anything else: "bad mask element (%f should be 0, 128 or 255)"), origin (mask_width / 2,
 * mask_height / 2); @morph is a VipsOperationMorphology (0 erode, 1 dilate).  The loops are over ELEMENTS and
 * bitwise: dilate ORs, erode ANDs, over the mask positions that are not 128, the input byte (255) or its complement
 * (0).  The input may have any non-complex format: it is vips_cast to uchar first (morph.c:866-870); the output is
 * uchar.  Masks up to 32 x 32 whose tile fits a CU's 160 KB of LDS (16 + mask_height - 1 rows of 1024 + (mask_width
 * - 1) * bands bytes: every mask up to 76 bands); others are refused.
 *
 * Both read, for output rows top .. top + height - 1, the input rows vips_hip_rank_need() names -- window_height / 2
 * above, the rest of the window below -- before they are clipped to the image (for vips_hip_morph_gen:
 * window_height = mask_height).  vips_hip_rank_step: the tiles of the kernels, for tests that want sizes round them
 * (0 / 1: elements of a row / rows a block of the rank kernels makes; 2 / 3: of the morph kernels; 4: the largest
 * mask side of vips_hip_morph_gen).
 */
VIPS_HIP_API int vips_hip_rank_gen(const VipsHipRegion *in, const VipsHipRegion *out, int width, int height, int index);
VIPS_HIP_API int vips_hip_morph_gen(const VipsHipRegion *in, const VipsHipRegion *out,
	const double *mask, int mask_width, int mask_height, int morph);
VIPS_HIP_API void vips_hip_rank_need(int window_height, int top, int height, int *in_top, int *in_height);
VIPS_HIP_API int vips_hip_rank_step(int what);

/* ---------------------------------------------------------- local histogram equalisation, statistical differencing
 *
 * The region forms of vips_hist_local and vips_stdif, in the shape of vips_hip_rank_gen: @in and @out are windows of
 * images of the same size and bands, both uchar (other formats: "image must be VIPS_FORMAT_UCHAR", the reference's words, with the format named); @in
 * holds what @out reads, clipped to the image.  Output element (x, y, b) looks at the @width x @height window whose
 * top-left is input pel (x - width / 2, y - height / 2), band b.  "window too large" when width > im_width or height >
 * im_height, in the reference's words.  Both read the rows vips_hip_rank_need() names (window_height = @height).
 *
 * vips_hist_local_generate (histogram/hist_local.c:142-270): the image is embedded with VIPS_EXTEND_MIRROR (:301-306:
 * reflected about its edge, the edge pel repeated; a window is never larger than the image, so a coordinate reflects
 * once, and a reflected row or column always lies inside the rows and columns named above).  t = the pel itself,
 * hist = the histogram of the window.  @max_slope 0: sum = the count of window elements <= t.  @max_slope 1 .. 100
 * (CLAHE, :211-238): sum = sum over v <= t of min(hist[v], max_slope) + (t + 1) * (what the clip took off all 256
 * bins) / 256, in int arithmetic in that order.  out = 255 * sum / (width * height), an int division.
 * Two kernel families: hist_local_count (max_slope 0 and width * height <= 64: compares over the tile in LDS, no
 * histogram) and hist_local_slide (everything else: the reference's sliding histogram, one a lane, 256 bins of 16
 * bits in LDS).  The sliding kernel takes windows of up to 65535 pels (a bin is 16 bits), 256 a side, up to 16 bands,
 * whose tile -- 8 + height - 1 rows of (16 / bands * 16 + width - 1) * bands bytes -- fits the 96 KB the bins leave of
 * a CU's LDS; what does not fit is refused with the sizes in the message.  vips_hip_hist_local_step: 0 the pels of a
 * run, 1 the rows a block of the sliding kernel makes (its tile is (3: lanes a row) / bands runs wide), 2 the largest
 * window side, 4 the largest window area of the counting kernel, 5 / 6 the elements of a row / rows a block of it makes.
 *
 * vips_stdif_generate (histogram/stdif.c:135-253): the image is embedded with VIPS_EXTEND_COPY (:284-289).  sum and
 * sum2 of the window are unsigned int; then, in double and in this order, with no fused multiply-add, correctly
 * rounded division and square root (:208-217): mean = sum / n, var = sum2 / n - mean * mean, sig = sqrt(var),
 * res = a * m0 + (1 - a) * mean + (t - mean) * (b * s0 / (s0 + b * sig)).  out = 0 for res < 0, 255 for res >= 256,
 * else (unsigned char) (res + 0.5) -- where 255.5 <= res < 256 converts 256.x to a byte: the reference's machine
 * (x86-64: cvttsd2si, then the low byte) stores 0, and so does the kernel.  s0 + b * sig == 0 divides by zero:
 * undefined, as in the reference.  Windows of more than 66051 pels are refused: above that sum2 wraps in the reference
 * and its result is its overflow.  One kernel, stdif_u8: column sums in LDS, then `width` of them an element.
 * vips_hip_stdif_step: 0 / 1 the elements of a row / rows (at most) a block makes, 2 the largest window area.
 */
VIPS_HIP_API int vips_hip_hist_local_gen(const VipsHipRegion *in, const VipsHipRegion *out, int width, int height, int max_slope);
VIPS_HIP_API int vips_hip_hist_local_step(int what);
VIPS_HIP_API int vips_hip_stdif_gen(const VipsHipRegion *in, const VipsHipRegion *out, int width, int height,
	double a, double m0, double b, double s0);
VIPS_HIP_API int vips_hip_stdif_step(int what);

/* ---------------------------------------------------------- edge detectors
 *
 * vips_sobel, vips_scharr and vips_prewitt (convolution/edge.c): a fixed 3 x 3 mask and its rot90 over the image,
 * the two results combined per element; any band count, the output is uchar.
 *   uchar input   vips_edge_build_uchar (edge.c:112-153): two integer convolutions with scale 2 and offset 128, each
 *                 rounded and clipped to 0 .. 255 as vips_convi_gen stores it, then |2 (c1 - 128)| + |2 (c2 - 128)|
 *                 saturated at 255 -- ONE kernel, one read of the image and one write (gate edge_u8).
 *   other input   vips_edge_build_float (:157-183): two float convolutions (each mask run as its own mask through the
 *                 kernels of vips_hip_conv_gen), then x * x + y * y in float, the square root in double, vips_cast to
 *                 uchar (gate edge_combine_f32).  char ... int and float; double and complex images are refused by
 *                 name.
 * (uchar images with the Highway arithmetic of convi selected, vips_hip_vector_set_enabled(), and pels too wide for
 * the fused kernel's tile take two vips_hip_conv_gen passes and the gate edge_combine_u8: the same pixels.)
 * The input window must hold the out rect grown by one pel all round, clipped to the image: rows
 * vips_hip_edge_need() names.  vips_hip_edge_step: 0 / 1 the elements of a row / the rows a block of the fused kernel
 * makes, 2 the widest pel (bands) it takes (3 .. 5: the same for vips_hip_canny_gen's kernel, below), 6 the most rows
 * the combining kernels (edge_combine_*, compass_combine) have in flight: their blocks take the other rows in turns.
 */
typedef enum {
	VIPS_HIP_EDGE_SOBEL = 0,
	VIPS_HIP_EDGE_SCHARR,
	VIPS_HIP_EDGE_PREWITT,
	VIPS_HIP_EDGE_LAST
} VipsHipEdge;
VIPS_HIP_API int vips_hip_edge_gen(const VipsHipRegion *in, const VipsHipRegion *out, int edge);
VIPS_HIP_API void vips_hip_edge_need(int top, int height, int *in_top, int *in_height);
VIPS_HIP_API int vips_hip_edge_step(int what);

/* vips_compass (convolution/compass.c): the image convolved with the mask `times` times, the mask turned by `angle`
 * (vips_rot45) between convolutions, the absolute values combined by max, min or sum.  The plan restates
 * vips_compass_build on the host: rot45 of an odd square matrix is pure index movement with period 8, so `times`
 * convolutions are at most eight distinct ones, each with a multiplicity (which only a sum sees).  A mask that is not
 * odd and square gives vips_rot45's error, "rot45: images must be odd and square".
 *   uchar, precision integer, a 3 x 3 mask   ONE kernel: every distinct mask's integer convolution, rounded, offset
 *                 and clipped as vips_convi_gen stores it, then max / min (uchar out) or the sum (uint out) -- one
 *                 read of the image, one write (gate compass_u8).
 *   everything else   every distinct mask through vips_hip_conv_gen / vips_hip_conva_gen as its own mask, then one
 *                 kernel for vips_abs and the combine over their results (gate compass_combine).  A float sum adds
 *                 its `times` terms in the reference's order.
 * The output format is what the reference's vips_bandrank / vips_sum make of the convolutions' format:
 * vips_hip_compass_out_format.  double and complex images are refused by name.  The input window must hold the out
 * rect grown by the mask (origin size / 2), clipped to the image: vips_hip_rank_need(size, ...) names its rows.
 */
typedef enum { /* VipsAngle45: steps of 45 degrees */
	VIPS_HIP_ANGLE45_D0 = 0,
	VIPS_HIP_ANGLE45_D45,
	VIPS_HIP_ANGLE45_D90,
	VIPS_HIP_ANGLE45_D135,
	VIPS_HIP_ANGLE45_D180,
	VIPS_HIP_ANGLE45_D225,
	VIPS_HIP_ANGLE45_D270,
	VIPS_HIP_ANGLE45_D315
} VipsHipAngle45;
typedef enum { /* VipsCombine */
	VIPS_HIP_COMBINE_MAX = 0,
	VIPS_HIP_COMBINE_SUM = 1,
	VIPS_HIP_COMBINE_MIN = 2
} VipsHipCombine;
typedef struct _VipsHipCompass VipsHipCompass;
/* vips_rot45 of a width x height matrix of doubles (host only, no device needed). */
VIPS_HIP_API int vips_hip_rot45(const double *in, int width, int height, int angle, double *out);
VIPS_HIP_API VipsHipCompass *vips_hip_compass_new(const double *mask, int mask_width, int mask_height, double scale,
	double offset, int times, int angle, int combine, int precision, int layers, int cluster);
VIPS_HIP_API void vips_hip_compass_free(VipsHipCompass *plan);
/* The distinct masks (each mask_width x mask_height doubles, the k-th one the mask turned k times) and how many of
 * the `times` convolutions run each; at most @max of them are written.  Returns their number (host only). */
VIPS_HIP_API int vips_hip_compass_get_masks(const VipsHipCompass *plan, double *masks, int *mult, int max);
VIPS_HIP_API int vips_hip_compass_out_format(const VipsHipCompass *plan, int format);
VIPS_HIP_API int vips_hip_compass_gen(const VipsHipCompass *plan, const VipsHipRegion *in, const VipsHipRegion *out);

/* vips_canny (convolution/canny.c) behind its blur: vips_canny_gradient (the 2 x 2 mask -1 1 / -1 1 and its rot90,
 * origin at (1, 1)), vips_canny_polar, the one-pel vips_embed(COPY) of the polar image and vips_canny_thin in ONE
 * kernel on a window of the BLURRED image (vips_hip_gaussblur makes it); any band count up to vips_hip_edge_step(5).
 *   a uchar blur (uchar input with precision integer or approximate)   integer gradients with offset 128 and their
 *                 clip, the 256-entry atan2 table (vips_hip_canny_table: vips_atan2_init's own expression on the
 *                 host), integer thinning; uchar out (gate canny_polar_thin_u8).
 *   any other blur (the default precision, float, turns every input into one)   float gradients as convf sums them,
 *                 POLAR(float) in double rounded to float, THIN(float) in float with every operation rounded; float
 *                 out (gate canny_polar_thin_f32).  double and complex images are refused by name.
 * Bit-identical to the reference but for one spot: theta is atan2 in double and the device's atan2 is not the host
 * library's; both are within a couple of ulp of the true value, so the floats can differ only where the double lies
 * within a few ulp of a float rounding boundary.  The float kernel COUNTS the pels whose theta would round to another
 * float had atan2's result been 4 ulp off either way: vips_hip_canny_marginal() returns that count for the calling
 * thread's device since it was last read (and clears it).  Zero means bit-identical.
 * vips_hip_canny's own blur always reproduces the reference's bits, whatever vips_hip_set_exact_float() says: the
 * gradient and the thinning turn a last bit of the blur into a decision.  vips_hip_canny_gen takes the blur its caller
 * made.
 * The window must hold the out rect grown by two pels above and to the left and one below and to the right, clipped
 * to the image: rows vips_hip_canny_need() names.  vips_hip_edge_step 3 / 4: the pels / rows a block makes.
 */
VIPS_HIP_API void vips_hip_canny_table(unsigned char *table);
VIPS_HIP_API void vips_hip_canny_need(int top, int height, int *in_top, int *in_height);
VIPS_HIP_API int vips_hip_canny_gen(const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API long long vips_hip_canny_marginal(void);

/* vips_sharpen_generate (convolution/sharpen.c:116-168): LabS in, LabS out; the
 * blurred L band comes from a vips_hip_conv_gen pass the caller ran.
 */
VIPS_HIP_API int vips_hip_sharpen_gen(const int *lut_device /* 65536 ints */,
	const VipsHipRegion *in, const VipsHipRegion *blurred_l, const VipsHipRegion *out);

/* --------------------------------------------------------------- image ops */

/* A whole image resident in HBM (the VipsImage of this library). */
typedef struct _VipsHipImage VipsHipImage;

VIPS_HIP_API VipsHipImage *vips_hip_image_new(int width, int height, int bands,
	int format, int interpretation);
/* Upload from / wrap host or device memory (vips_image_new_from_memory,
 * iofuncs/image.c). */
VIPS_HIP_API VipsHipImage *vips_hip_image_new_from_memory(const void *host_data,
	int width, int height, int bands, int format, int interpretation);
VIPS_HIP_API VipsHipImage *vips_hip_image_new_from_device(void *device_data,
	int width, int height, int bands, int format, int interpretation);
VIPS_HIP_API void vips_hip_image_unref(VipsHipImage *image);
/* vips_hip_image_unref() on images[0 .. n) (NULL entries are skipped), each entry set to NULL:
 * what a caller of the batch entry points does with a batch's results (VIPS_UNREF in a loop,
 * g_object_unref, gobject/gobject.c). */
VIPS_HIP_API void vips_hip_image_unref_many(VipsHipImage **images, int n);
VIPS_HIP_API int vips_hip_image_write_to_memory(const VipsHipImage *image, void *host_data);
VIPS_HIP_API void *vips_hip_image_get_data(const VipsHipImage *image);
/* the device the pixels live on (-1 for a NULL image) */
VIPS_HIP_API int vips_hip_image_get_device(const VipsHipImage *image);
VIPS_HIP_API int vips_hip_image_get_width(const VipsHipImage *image);
VIPS_HIP_API int vips_hip_image_get_height(const VipsHipImage *image);
VIPS_HIP_API int vips_hip_image_get_bands(const VipsHipImage *image);
VIPS_HIP_API int vips_hip_image_get_format(const VipsHipImage *image);
VIPS_HIP_API int vips_hip_image_get_interpretation(const VipsHipImage *image);
VIPS_HIP_API size_t vips_hip_image_get_stride(const VipsHipImage *image);
VIPS_HIP_API void vips_hip_image_region(const VipsHipImage *image, VipsHipRegion *region);
/* The EXIF-style orientation, the one piece of metadata an image carries: 1 .. 8, or 0 for an image that has none
 * (read as 1, as vips_image_get_orientation does).  Images made by the constructors above have none; the JPEG
 * loader sets it from the EXIF tag and the .v loader from the file's metadata.  vips_hip_rot and vips_hip_flip
 * carry it through unchanged (as the reference does), vips_hip_autorot acts on it and clears it, the
 * vips_hip_thumbnail*_rotate entry points act on it or keep it; EVERY OTHER operation's result has none.
 */
VIPS_HIP_API int vips_hip_image_get_orientation(const VipsHipImage *image);
VIPS_HIP_API int vips_hip_image_set_orientation(VipsHipImage *image, int orientation);

/* The native ".v" format (doc/file-format.md; iofuncs/vips.c:283-441): 64-byte header, then
 * band-interleaved scanlines without padding, then optional XML metadata (iofuncs/vips.c:560-622), of which the
 * orientation is carried and nothing else: the loader reads <field type="gint" name="orientation"> inside <meta>, the
 * saver appends a trailer with that one field to an image that has an orientation, and to no other (such a file is
 * header + pixels).  vips_hip_vfile_read_orientation is host-only: 0 for a file without one.
 * vips_hip_vfile_read_header is host-only (vips__read_header_bytes plus the file-length check of
 * iofuncs/image.c:966-979); the loader and the saver move the pixels between the file and HBM
 * through two pinned buffers so that disc and PCIe transfers overlap (the role of the two
 * write-behind buffers of iofuncs/sinkdisc.c:195-220).  Files with big-endian pixels or LABQ /
 * RAD coding are refused.
 */
typedef struct _VipsHipVHeader {
	int width, height, bands;
	int format;         /* VipsBandFormat */
	int coding;         /* VipsCoding: 0 none, 2 LABQ, 6 RAD */
	int interpretation; /* VipsInterpretation, -1 when the file holds an unknown value */
	float xres, yres;   /* pixels per mm */
	int xoffset, yoffset;
	int msb_first;         /* pixel data is big-endian */
	long long data_offset; /* == 64 */
	long long data_size;   /* width * height * bands * sizeof(format) */
} VipsHipVHeader;

VIPS_HIP_API int vips_hip_vfile_read_header(const char *path, VipsHipVHeader *header);
VIPS_HIP_API int vips_hip_vfile_read_orientation(const char *path, int *orientation);
VIPS_HIP_API VipsHipImage *vips_hip_image_new_from_vfile(const char *path);
VIPS_HIP_API int vips_hip_image_write_to_vfile(const VipsHipImage *image, const char *path);

/* JPEG shrink-on-load in front of the device path.  The entropy decode is
 * libjpeg's, on the host, exactly as foreign/jpeg2vips.c:517-640,800-905 drives it (scale 1/shrink,
 * output cropped to size / shrink rounded down, CMYK inverted); libjpeg.so.9 is bound with dlopen
 * at first use.  vips_hip_thumbnail is vips_thumbnail() (resample/thumbnail.c:549-676 open +
 * :678-1067 build) for JPEG and .v files: vips_thumbnail_find_jpegshrink (:488-519) picks the
 * block shrink, the pre-shrunk image is uploaded, the rest is vips_hip_thumbnail_image.  Files
 * that need ICC colour management (an embedded profile in linear mode) are refused.
 *
 * Auto-rotation: the *_rotate entry points are vips_thumbnail with its no_rotate argument.  With @no_rotate 0
 * an orientation that swaps the axes (5 .. 8) swaps the target box for the shrink calculation (thumbnail.c:416-420,
 * vips_hip_thumbnail_find_jpegshrink_rotate's @swap), vips_autorot runs after the conversion back to the output
 * space and before the crop (:989-1062), and the result has no orientation; with @no_rotate 1 the pixels stay as
 * stored and the result keeps the tag.  The entry points without the argument are as they were before there was
 * auto-rotation: vips_hip_thumbnail refuses a JPEG whose orientation is not 1 and ignores a .v file's.
 */
typedef struct _VipsHipJpegHeader {
	int width, height;             /* after the shrink */
	int bands;                     /* 1 grey, 3 RGB, 4 CMYK */
	int interpretation;            /* B_W, sRGB or CMYK (15) */
	int image_width, image_height; /* of the file */
	int orientation;               /* EXIF orientation, 0 when absent */
	int has_icc;
} VipsHipJpegHeader;

VIPS_HIP_API int vips_hip_thumbnail_find_jpegshrink(int in_width, int in_height,
	int width, int height, int size, int linear, int crop);
VIPS_HIP_API int vips_hip_thumbnail_find_jpegshrink_rotate(int in_width, int in_height,
	int width, int height, int size, int linear, int crop, int swap);
VIPS_HIP_API int vips_hip_jpeg_read_header(const char *path, int shrink, VipsHipJpegHeader *header);
VIPS_HIP_API int vips_hip_jpeg_read_to_memory(const char *path, int shrink, void *host_data, size_t size);
VIPS_HIP_API VipsHipImage *vips_hip_image_new_from_jpeg(const char *path, int shrink);
VIPS_HIP_API int vips_hip_thumbnail(const char *path, VipsHipImage **out,
	int width, int height, int size, int linear, int crop);
VIPS_HIP_API int vips_hip_thumbnail_rotate(const char *path, VipsHipImage **out,
	int width, int height, int size, int linear, int crop, int no_rotate);
/* @n files on @n_threads host threads, each with its own stream: decode, upload and device work
 * of different files overlap (the shape of BASELINE config C4 when the inputs are files).
 * Returns the number of failures; outs[i] is NULL for those and, when @errors is given
 * (n x 256 bytes), errors + 256 * i holds the message.
 */
VIPS_HIP_API int vips_hip_thumbnail_batch(const char *const *paths, int n, VipsHipImage **outs,
	char *errors, int width, int height, int size, int linear, int crop, int n_threads);
VIPS_HIP_API int vips_hip_thumbnail_batch_rotate(const char *const *paths, int n, VipsHipImage **outs,
	char *errors, int width, int height, int size, int linear, int crop, int no_rotate, int n_threads);

/* Emulate the reference sink's strip height when seeding the reduce position
 * accumulators (see vips_hip_reducev_gen_tiled); default 16 = vips__fatstrip_height
 * (include/vips/private.h:147-153). */
VIPS_HIP_API void vips_hip_set_fatstrip_height(int lines);

/* The operation wrappers: same names, argument meaning and error behaviour as
 * vips_reduceh() .. vips_thumbnail_image(); optional arguments are explicit.
 * On success *out is a new image the caller unrefs.
 */
VIPS_HIP_API int vips_hip_reduceh(VipsHipImage *in, VipsHipImage **out,
	double hshrink, int kernel, double gap);
VIPS_HIP_API int vips_hip_reducev(VipsHipImage *in, VipsHipImage **out,
	double vshrink, int kernel, double gap);
VIPS_HIP_API int vips_hip_reduce(VipsHipImage *in, VipsHipImage **out,
	double hshrink, double vshrink, int kernel, double gap);
VIPS_HIP_API int vips_hip_shrinkh(VipsHipImage *in, VipsHipImage **out, int hshrink, int ceil_mode);
VIPS_HIP_API int vips_hip_shrinkv(VipsHipImage *in, VipsHipImage **out, int vshrink, int ceil_mode);
VIPS_HIP_API int vips_hip_shrink(VipsHipImage *in, VipsHipImage **out,
	double hshrink, double vshrink, int ceil_mode);
/* vips_resize (resample/resize.c:135-329): integer shrink + reduce for scales < 1, vips_affine
 * with the kernel's interpolator (or vips_zoom) for scales > 1; vscale <= 0 means == scale;
 * gap < 0 selects the default 2.0 (resize.c:397).  Kernel nearest shrinks by vips_subsample
 * first (resize.c:165-203). */
VIPS_HIP_API int vips_hip_resize(VipsHipImage *in, VipsHipImage **out,
	double scale, double vscale, int kernel, double gap);
/* vips_thumbnail_image (resample/thumbnail.c:678-1067 with vips_thumbnail_calculate_shrink
 * :413-467): processing-space conversion, the shrink for the target box and fit mode,
 * vips_resize, conversion back.  @height <= 0 means == @width; @size is a VipsSize
 * (include/vips/resample.h: 0 both, 1 up, 2 down, 3 force); @linear shrinks in scRGB.
 * Images with alpha are premultiplied around the resize (thumbnail.c:848-904).  This entry point does not look
 * at the image's orientation (vips_hip_thumbnail_image_rotate does); ICC is outside the path.
 */
VIPS_HIP_API int vips_hip_thumbnail_image(VipsHipImage *in, VipsHipImage **out,
	int width, int height, int size, int linear);
/* ... with the crop argument (a VipsInteresting, include/vips/conversion.h:97-107): the box is
 * filled instead of fitted (thumbnail.c:432-437) and the result cut to it by vips_smartcrop's
 * modes (vips_hip_smartcrop below): 0 none, 1 centre, 2 entropy, 3 attention, 4 low, 5 high, 6 all.
 */
VIPS_HIP_API int vips_hip_thumbnail_image_crop(VipsHipImage *in, VipsHipImage **out,
	int width, int height, int size, int linear, int crop);
/* ... with vips_thumbnail's auto-rotation by the image's orientation (see vips_hip_thumbnail_rotate above). */
VIPS_HIP_API int vips_hip_thumbnail_image_rotate(VipsHipImage *in, VipsHipImage **out,
	int width, int height, int size, int linear, int crop, int no_rotate);
/* vips_rot / vips_flip (@angle, @direction as in vips_hip_rot_gen; d0 shares the pixels) and vips_autorot
 * (conversion/autorot.c:103-191): the turn and flip that undo the image's orientation, as ONE launch; the result
 * has no orientation; @angle (a VipsAngle) and @flip say what was done and may be NULL. */
VIPS_HIP_API int vips_hip_rot(VipsHipImage *in, VipsHipImage **out, int angle);
VIPS_HIP_API int vips_hip_flip(VipsHipImage *in, VipsHipImage **out, int direction);
VIPS_HIP_API int vips_hip_autorot(VipsHipImage *in, VipsHipImage **out, int *angle, int *flip);
/* vips_extract_area (conversion/extract.c:137-187). */
VIPS_HIP_API int vips_hip_extract_area(VipsHipImage *in, VipsHipImage **out,
	int left, int top, int width, int height);
/* vips_hist_find (arithmetic/hist_find.c) of a uchar image of 1 .. 4 bands: @band -1 counts every band, else
 * the one band.  The result is a UINT image one row high, mx + 1 pels wide -- mx the largest value a counted
 * band holds; 255 when every band is counted (hist_find.c:175-178, 350-394) -- of interpretation HISTOGRAM.
 * Other formats (what the reference would cast) and images of 2^31 pels or more are refused. */
VIPS_HIP_API int vips_hip_hist_find(VipsHipImage *in, VipsHipImage **out, int band);
/* The kernel under it: the histograms of @n (1 .. 6) rectangles of @in -- @rects holds left, top, width, height
 * for each -- in ONE launch and one copy back; @counts (host memory) takes 256 * bands counters a rectangle,
 * the count of value v in band b at [v * bands + b].  vips_hip_hist_step: what the kernel takes at a time, for
 * tests that want sizes round it (0: the bytes of a row a wave takes in a step; 1: the rows a block takes; 2 / 3:
 * the most blocks a histogram launch, all rectangles together, / a vips_hip_maplut launch has: a wave takes the rows
 * beyond them in turns). */
VIPS_HIP_API int vips_hip_hist_rects(VipsHipImage *in, const int *rects, int n, unsigned int *counts);
VIPS_HIP_API int vips_hip_hist_step(int what);
/* vips_maplut (histogram/maplut.c:612-760) of a uchar image: out = lut[in], band by band.  @lut is an image one row
 * or one column of n <= 256 entries (vips_check_hist's messages; more entries are index formats this path does not
 * have: refused), any non-complex format, of 1 band, of @in's bands, or of any bands when @in has one.  An index
 * above n - 1 reads entry n - 1 (maplut.c's clp).  The output has the LUT's format, and the LUT's bands unless the LUT
 * has one band, then @in's.  @band >= 0 with a one-band LUT maps that band and sends the others through the identity
 * of n entries (PACK_TABLE, :562-581: they are clipped to n - 1 too); -1 otherwise.
 * Interpretation (:656-669): the LUT's when it has more than one band, else @in's; then vips_image_guess_interpretation
 * of the result: a tag that cannot be true of it -- MULTIBAND always, HISTOGRAM on an image more than one pel wide and
 * high, 16-bit tags on 8-bit pels, fewer bands than the tag needs -- gives way to the default for the format and bands
 * (B_W / sRGB, GREY16 / RGB16 for ushort, MULTIBAND above four bands).
 * One kernel, maplut_u8: the table (at most 256 x 4 bands x 8 bytes, larger ones are refused) in LDS, 16-byte loads
 * of the input, whole-dword stores. */
VIPS_HIP_API int vips_hip_maplut(VipsHipImage *in, VipsHipImage *lut, VipsHipImage **out, int band);
/* vips_hist_cum (histogram/hist_cum.c:72-167) and vips_hist_norm (hist_norm.c:74-125) of the one-row UINT histograms
 * vips_hip_hist_find and vips_hip_hist_cum make (other images are refused, with their format in the message).  A
 * histogram is 256 x bands numbers: downloaded, worked out on the host, uploaded; no kernel.  The *_host forms are the
 * arithmetic alone, on @width pels of @bands counters in host memory.  hist_norm restates the reference step by step:
 * vips_stats' maximum of each band; a = (width - 1) / max in double; vips_linear -- a[k] * (float) p[i] + b[k] stored as
 * a float (LOOPN, arithmetic/linear.c:227-236), or, when every band has the same maximum, the constants as floats and
 * float arithmetic (LOOP1, :213-223) -- so counts above 2^24 lose the bits the reference loses; vips_cast to the
 * smallest unsigned format that holds width - 1 (uchar up to 256 pels), which vips_hip_hist_norm_host returns (-1 for a null argument); @out
 * takes elements of that format.  A band of zeros divides by zero: undefined. */
VIPS_HIP_API int vips_hip_hist_cum(VipsHipImage *in, VipsHipImage **out);
VIPS_HIP_API int vips_hip_hist_norm(VipsHipImage *in, VipsHipImage **out);
VIPS_HIP_API void vips_hip_hist_cum_host(const unsigned int *in, int width, int bands, unsigned int *out);
VIPS_HIP_API int vips_hip_hist_norm_host(const unsigned int *in, int width, int bands, void *out);
/* vips_hist_equal (hist_equal.c:74-98): hist_find(@band) -> hist_cum -> hist_norm -> cast to the input's format ->
 * maplut, for uchar images of 1 .. 4 bands (vips_hip_hist_find's limits; others are refused by name).  @band -1: every
 * band through its own table; @band k: the one table of band k, mx + 1 entries wide, on every band with the clip.
 * Two launches an image -- the histogram kernel and maplut_u8 -- and one round trip of 1 KB a band between them. */
VIPS_HIP_API int vips_hip_hist_equal(VipsHipImage *in, VipsHipImage **out, int band);
/* vips_hist_local (hist_local.c:272-333) and vips_stdif (stdif.c:255-320) on whole images: see
 * vips_hip_hist_local_gen / vips_hip_stdif_gen above.  The result has the size, bands and interpretation of the input.
 * The class defaults: max_slope 0; a 0.5, m0 128, b 0.5, s0 50. */
VIPS_HIP_API int vips_hip_hist_local(VipsHipImage *in, VipsHipImage **out, int width, int height, int max_slope);
VIPS_HIP_API int vips_hip_stdif(VipsHipImage *in, VipsHipImage **out, int width, int height,
	double a, double m0, double b, double s0);
/* vips_smartcrop (conversion/smartcrop.c:322-437): @width x @height pels of @in, placed by @interesting (a
 * VipsInteresting: 0 none, 1 centre, 2 entropy, 3 attention, 4 low, 5 high, 6 all).  @left, @top (where the
 * crop was taken), @attention_x, @attention_y (the point the attention mode found; 0 for the others) may be NULL.
 * entropy (smartcrop.c:106-176) takes uchar images of 1 or 3 bands: up to 8 rounds, each ONE launch of the
 * histogram kernel over the six slices the round can ask about and one copy back; the slices' entropies
 * (histogram/hist_entropy.c:61-95) are worked out on the host from the counters, step by step as the reference
 * does.  attention (smartcrop.c:204-320) takes uchar images of 3 bands that vips_hip_colourspace takes to XYZ.
 * Images with alpha, other formats and one-band attention are refused, with the mode's name in the message. */
VIPS_HIP_API int vips_hip_smartcrop(VipsHipImage *in, VipsHipImage **out, int width, int height, int interesting,
	int *left, int *top, int *attention_x, int *attention_y);
/* vips_rank (morphology/rank.c:458-539), vips_median (:639-671: rank(size, size, size * size / 2)) and vips_morph
 * (morph.c:828-941) on whole images: see vips_hip_rank_gen / vips_hip_morph_gen above for what they compute, take and
 * refuse.  The result has the size of the input; vips_hip_morph's is uchar. */
VIPS_HIP_API int vips_hip_rank(VipsHipImage *in, VipsHipImage **out, int width, int height, int index);
VIPS_HIP_API int vips_hip_median(VipsHipImage *in, VipsHipImage **out, int size);
VIPS_HIP_API int vips_hip_morph(VipsHipImage *in, VipsHipImage **out,
	const double *mask, int mask_width, int mask_height, int morph);
/* vips_sobel, vips_scharr, vips_prewitt (convolution/edge.c) on whole images: see vips_hip_edge_gen above.  The
 * result has the size and bands of the input and is uchar. */
VIPS_HIP_API int vips_hip_sobel(VipsHipImage *in, VipsHipImage **out);
VIPS_HIP_API int vips_hip_scharr(VipsHipImage *in, VipsHipImage **out);
VIPS_HIP_API int vips_hip_prewitt(VipsHipImage *in, VipsHipImage **out);
/* vips_canny (canny.c:380-429): vips_hip_gaussblur(sigma, precision), then vips_hip_canny_gen on the blurred image.
 * The class defaults: sigma 1.4, precision float. */
VIPS_HIP_API int vips_hip_canny(VipsHipImage *in, VipsHipImage **out, double sigma, int precision);
/* vips_compass on a whole image: see vips_hip_compass_gen above (the class defaults: times 2, angle d90, combine max,
 * precision float, layers 5, cluster 1). */
VIPS_HIP_API int vips_hip_compass(VipsHipImage *in, VipsHipImage **out, const double *mask, int mask_width, int mask_height,
	double scale, double offset, int times, int angle, int combine, int precision, int layers, int cluster);
VIPS_HIP_API int vips_hip_conv(VipsHipImage *in, VipsHipImage **out,
	const double *mask, int mask_width, int mask_height, double scale, double offset,
	int precision);
VIPS_HIP_API int vips_hip_convsep(VipsHipImage *in, VipsHipImage **out,
	const double *mask, int mask_n, double scale, double offset, int precision);
/* vips_conva (conva.c:1231-1280) / vips_convasep (convasep.c:775-828): what vips_conv /
 * vips_convsep / vips_gaussblur run for precision APPROXIMATE (with layers 5, cluster 1). */
VIPS_HIP_API int vips_hip_conva(VipsHipImage *in, VipsHipImage **out,
	const double *mask, int mask_width, int mask_height, double scale, double offset,
	int layers, int cluster);
VIPS_HIP_API int vips_hip_convasep(VipsHipImage *in, VipsHipImage **out,
	const double *mask, int mask_n, double scale, double offset, int layers);
VIPS_HIP_API int vips_hip_gaussblur(VipsHipImage *in, VipsHipImage **out,
	double sigma, double min_ampl, int precision);
VIPS_HIP_API int vips_hip_sharpen(VipsHipImage *in, VipsHipImage **out,
	double sigma, double x1, double y2, double y3, double m1, double m2);
/* ------------------------------------------------- row strips over the devices of one process
 *
 * BASELINE config 5 (vips_conv 31 x 31 on 65536 x 65536 ushort tiled across 8 GPUs) the way
 * libvips itself is parallel: threads of ONE process (iofuncs/threadpool.c:301-373, 625), here a
 * thread per device.  An image is held as n row strips, strip k in a persistent window on
 * devices[k] with room for `halo` rows of its neighbours above and below;
 * vips_hip_strips_exchange() moves every halo row device to device (hipMemcpyPeerAsync, xGMI)
 * straight into the window that needs it; vips_hip_conv_strips() = that exchange + the region
 * operation vips_hip_conv_gen() on every window at once.  Pixels are the single-device result's
 * bit for bit.  (The one-process-per-GPU form of the same partition, halos over RCCL, is
 * libvips_amd/sharding.py.)
 */
typedef struct _VipsHipStrips VipsHipStrips;
VIPS_HIP_API VipsHipStrips *vips_hip_strips_new(int im_width, int im_height, int bands, int format,
	int n, const int *devices, int halo);
VIPS_HIP_API void vips_hip_strips_free(VipsHipStrips *strips);
VIPS_HIP_API int vips_hip_strips_count(const VipsHipStrips *strips);
/* strip k: its device, the region of its own rows and the region of its whole window (own rows +
 * halos), both in image coordinates, pointing into the window (fill `own`, read `window`) */
VIPS_HIP_API int vips_hip_strips_region(const VipsHipStrips *strips, int k, int *device,
	VipsHipRegion *own, VipsHipRegion *window);
/* the own rows must be complete (synchronised) on entry; the halos are complete on return */
VIPS_HIP_API int vips_hip_strips_exchange(VipsHipStrips *strips);
/* out[0 .. n): strip k of vips_conv(image), an image on devices[k] */
VIPS_HIP_API int vips_hip_conv_strips(VipsHipStrips *strips, VipsHipImage **out, const double *mask,
	int mask_width, int mask_height, double scale, double offset, int precision);

/* BASELINE config 4: vips_resize(scale, kernel, gap) [then vips_sharpen(sigma, x1, y2, y3, m1,
 * m2)] on n independent images, as libvips would run n pipelines over its thread pool
 * (iofuncs/threadpool.c:625).  A batch of same-sized uchar images whose resize is by 1 / (2 k)
 * runs as one launch of the whole resize chain and one of the sharpen per 64 images; any
 * other batch on n_threads host threads that take images in turn, each on its own stream.
 * sigma < 0: no sharpen.  Returns the number of images that failed (out[i] NULL), -1 when
 * the batch failed as a whole (every out[i] NULL); everything is complete on return.
 */
VIPS_HIP_API int vips_hip_resize_sharpen_batch(VipsHipImage *const *in, int n, VipsHipImage **out,
	double scale, int kernel, double gap,
	double sigma, double x1, double y2, double y3, double m1, double m2, int n_threads);
/* The same, QUEUED: a batch the library runs in batch launches on the caller's device (same-sized
 * uchar images, a 1 / (2 k) resize) returns as soon as its work is queued -- the results are
 * ordered on the calling thread's stream like those of every single-image operation (use them in
 * stream order, or vips_hip_synchronize()) and the host can prepare the next batch meanwhile: what
 * libvips' pipelines do between a sink's two buffers (iofuncs/sinkdisc.c:177-220).  Any other
 * batch, and any failure, completes before the return as above. */
VIPS_HIP_API int vips_hip_resize_sharpen_batch_queue(VipsHipImage *const *in, int n, VipsHipImage **out,
	double scale, int kernel, double gap,
	double sigma, double x1, double y2, double y3, double m1, double m2, int n_threads);
VIPS_HIP_API int vips_hip_colourspace(VipsHipImage *in, VipsHipImage **out, int space);
/* vips_gaussblur() then vips_colourspace() (convolution/gaussblur.c:71-116,
 * colour/colourspace.c:551-612) as one call: on 3-band float images both blur passes and
 * the colour route run in one streaming kernel and the blurred image never reaches HBM
 * (BASELINE config 3); other images take the two operations.  Same pixels either way.
 * The libvips module calls this when a colourspace_hip consumes a gaussblur_hip that nobody
 * has evaluated yet.
 */
VIPS_HIP_API int vips_hip_gaussblur_colourspace(VipsHipImage *in, VipsHipImage **out,
	double sigma, double min_ampl, int precision, int space);
VIPS_HIP_API int vips_hip_cast(VipsHipImage *in, VipsHipImage **out, int format);
/* vips_premultiply / vips_unpremultiply with max_alpha from the interpretation
 * (premultiply.c:246-250) and alpha = the last band. */
VIPS_HIP_API int vips_hip_premultiply(VipsHipImage *in, VipsHipImage **out, int uchar);
VIPS_HIP_API int vips_hip_unpremultiply(VipsHipImage *in, VipsHipImage **out, int uchar);

/* ------------------------------------------------ affine / similarity / rotate
 *
 * vips_affine (resample/affine.c:226-625) with the nearest / bilinear / bicubic interpolators, any matrix, every
 * `extend`, `background`, `oarea`, `odx` / `ody` / `idx` / `idy` and `premultiplied`; vips_similarity and vips_rotate
 * (resample/similarity.c:83-111) make their matrix and run it.  uchar ... int and float images of pels up to
 * VIPS_HIP_AFFINE_MAX_PEL bytes; double and complex images and every other interpolator are refused by name.
 */
typedef enum { /* VipsExtend, include/vips/conversion.h */
	VIPS_HIP_EXTEND_BLACK = 0,
	VIPS_HIP_EXTEND_COPY = 1,
	VIPS_HIP_EXTEND_REPEAT = 2,
	VIPS_HIP_EXTEND_MIRROR = 3,
	VIPS_HIP_EXTEND_WHITE = 4,
	VIPS_HIP_EXTEND_BACKGROUND = 5
} VipsHipExtend;

#define VIPS_HIP_AFFINE_MAX_PEL 64
#define VIPS_HIP_AFFINE_MAX_BACKGROUND 64

/* The arguments of vips_affine.  vips_hip_affine_defaults() sets the operation's defaults: the identity matrix,
 * bilinear, extend background, background 0, no oarea (the bounding box of the transformed image is used). */
typedef struct {
	double a, b, c, d;
	double odx, ody, idx, idy;
	int oarea[4]; /* left, top, width, height */
	int have_oarea;
	int interpolate; /* VipsHipInterpolate; any other value is refused */
	int extend;      /* VipsHipExtend */
	int premultiplied;
	int force_tiles;  /* the input comes from a SMALLTILE pipeline: 128-column rects even for a pure scale */
	int n_background; /* 1 or the band count */
	double background[VIPS_HIP_AFFINE_MAX_BACKGROUND];
} VipsHipAffine;
VIPS_HIP_API void vips_hip_affine_defaults(VipsHipAffine *args);

/* vips_affine_build restated for an input image of the given header: the inverse ("singular or near-singular
 * matrix"), the default oarea, the identity shortcut, the range check ("output coordinates out of range"), the ink
 * ("linear: vector must have 1 or N elements").  No pixel moves and no device is touched.  An image with alpha (by
 * its interpretation and bands, vips_image_hasalpha) and premultiplied == 0 is resampled as the float image
 * vips_premultiply makes of it: the plan's regions are then float.
 * vips_hip_affine_plan_get: 0 / 1 output width / height, 2 the transform is the identity copy, 3 the rect grid the
 * reference's demand hint gives for an image from memory (0: whole rows, b == c == 0 and an extend other than repeat
 * and mirror, whose embed is tiled; else 128), 4 the regions are the premultiplied float
 * image's, 5 the format of the regions. */
typedef struct _VipsHipAffinePlan VipsHipAffinePlan;
VIPS_HIP_API VipsHipAffinePlan *vips_hip_affine_plan_new(const VipsHipAffine *args, int width, int height, int bands,
	int format, int interpretation);
VIPS_HIP_API void vips_hip_affine_plan_free(VipsHipAffinePlan *plan);
VIPS_HIP_API int vips_hip_affine_plan_get(const VipsHipAffinePlan *plan, int what);
/* The rect of the input image that the output rect (left, top, width, height) reads (affine.c:267-303), clipped to
 * the image; in[2] or in[3] is 0 when the rect is all background. */
VIPS_HIP_API void vips_hip_affine_need(const VipsHipAffinePlan *plan, int left, int top, int width, int height, int in[4]);
/* vips_affine_gen (affine.c:226-410): fills @out's rect of the output image from @in, a window of the (premultiplied)
 * input image that must cover vips_hip_affine_need() of the rect ("input region too small" otherwise; for an
 * all-background rect any window will do).  The reference accumulates a row's coordinates from the first pixel of
 * each generate rect: @tile_width says where those rects start (multiples of it on the output image's own grid, up
 * to 1024; 0 = whole rows, which needs b == c == 0).  The accumulation is replayed on the device, add by add. */
VIPS_HIP_API int vips_hip_affine_gen(VipsHipAffinePlan *plan, const VipsHipRegion *in, const VipsHipRegion *out,
	int tile_width);
/* Whole images; the premultiply / unpremultiply / cast chain of affine.c:546-619 included. */
VIPS_HIP_API int vips_hip_affine(VipsHipImage *in, VipsHipImage **out, const VipsHipAffine *args);
/* @args: everything but the matrix (NULL: the defaults). */
VIPS_HIP_API int vips_hip_similarity(VipsHipImage *in, VipsHipImage **out, double scale, double angle,
	const VipsHipAffine *args);
VIPS_HIP_API int vips_hip_rotate(VipsHipImage *in, VipsHipImage **out, double angle, const VipsHipAffine *args);

/* ------------------------------------------------ mapim and xyz
 *
 * vips_mapim (resample/mapim.c): output pel (x, y) is the input resampled at the coordinate that pel (x, y) of @index
 * holds.  The index has two bands of any non-complex format, or one complex band (real part x); the result has the
 * index's size and the input's bands, format and interpretation.  Images are what vips_affine takes here: uchar ... int
 * and float, pels of up to VIPS_HIP_AFFINE_MAX_PEL bytes, the nearest / bilinear / bicubic interpolators, every
 * `extend`; double and complex images and every other interpolator are refused by name, and so is a complex index of
 * more than one band (the reference takes it and reads every second pel of it).
 * An index component is turned into a coordinate in the arithmetic of its own type (mapim.c:228-305): integers as
 * integers, float and complex in float -- (x + window_offset) + 1, each sum rounded to float --, double in double.
 * A pel whose index holds a NaN, lies below -1 or at or beyond size + 1 is the background ink.
 */
typedef struct {
	int interpolate; /* VipsHipInterpolate; any other value is refused */
	int extend;      /* VipsHipExtend */
	int premultiplied;
	int n_background; /* 1 or the band count */
	double background[VIPS_HIP_AFFINE_MAX_BACKGROUND];
} VipsHipMapim;
/* bilinear, extend background, background 0, not premultiplied */
VIPS_HIP_API void vips_hip_mapim_defaults(VipsHipMapim *args);
/* Whole images, the premultiply / unpremultiply / cast chain of mapim.c:482-531 included: an image with alpha (by its
 * interpretation and bands) and premultiplied == 0 is resampled as the float image vips_premultiply makes of it. */
VIPS_HIP_API int vips_hip_mapim(VipsHipImage *in, VipsHipImage *index, VipsHipImage **out, const VipsHipMapim *args);
/* vips_mapim_region_minmax and the need of vips_mapim_gen (mapim.c:145-224, :351-365) for a rect of the index, an image
 * in device memory: one read-only launch and 16 bytes back.  need[] is the rect of the input image (in_width x
 * in_height) that the rect reads, clipped to it, as vips_hip_affine_need reports it; need[2] or need[3] is 0 when
 * every pel of the rect is ink.  Components that are NaN are skipped.  (The reference starts its scan from the rect's
 * FIRST pel whatever it holds: for a rect that starts with a NaN its answer is its machine's, and differs from this
 * one.  The pixels do not depend on it.) */
VIPS_HIP_API int vips_hip_mapim_need(const VipsHipRegion *index_region, const VipsHipMapim *args, int in_width, int in_height,
	int need[4]);
/* The host half of the above: bounds[] = min x, min y, max x, max y of the index's components as doubles; floor /
 * ceil, the clip to [-1, VIPS_MAX_COORD], the stencil, the offset of 1, the intersection with the embedded image. */
VIPS_HIP_API int vips_hip_mapim_bounds_need(const double bounds[4], const VipsHipMapim *args, int in_width, int in_height,
	int need[4]);
/* vips_mapim_gen (mapim.c:307-428) on regions, which may be strided windows of larger frames: @out_region and
 * @index_region are the same rect of the output and of the index, @in_region a window of the in_width x in_height
 * input that must cover vips_hip_mapim_need() of the rect ("input region too small" otherwise: the bounds pass runs to
 * check, unless the window is the whole image; an all-ink rect accepts any window).  The regions' image is resampled
 * as it is -- no premultiply chain -- and extend white paints 255. */
VIPS_HIP_API int vips_hip_mapim_gen(const VipsHipRegion *in_region, const VipsHipRegion *index_region,
	const VipsHipRegion *out_region, const VipsHipMapim *args, int in_width, int in_height);
/* The kernels' units, for tests that want sizes round them: 0 / 1 the pels / rows of a block's patch of the output,
 * 2 / 3 of a wave's patch, 4 the most blocks a bounds launch has, 5 the threads of a block of the bounds and xyz
 * kernels, 6 the bytes of a group of the xyz kernel, 7 the most blocks an xyz launch has (its lanes take the other
 * groups in turns; the bounds pass shares these blocks out between a row's pels and the rows); -1 for anything else. */
VIPS_HIP_API int vips_hip_mapim_step(int what);
/* vips_xyz (create/xyz.c) in two dimensions: a two-band uint image of interpretation multiband whose pel (x, y) holds
 * (x, y), made on the device. */
VIPS_HIP_API int vips_hip_xyz(VipsHipImage **out, int width, int height);

/* ------------------------------------------------ template matching: fastcor, spcor
 *
 * vips_fastcor and vips_spcor (convolution/fastcor.c, spcor.c, correlation.c): @ref is slid over @in.  @out has the size
 * and the interpretation of @in (of @ref where a one-band @in is matched to its bands); the two are brought to a
 * common format (vips__formatalike) and to common bands (vips__bandalike: one band against n, "not one band or n
 * bands" otherwise).  @in is extended by copies of its edges and
 * sits at (ref.width / 2, ref.height / 2) of a canvas of in.size + ref.size - 1: output pel (x, y) compares @ref with
 * the window of that canvas whose top-left corner is (x, y).  The canvas is not made.
 *   fastcor: the sum of squared differences.  uint for integer images (the sum modulo 2^32), float for float, double for
 *            double (sum = sum + dif * dif in the type, rows of the ref, then columns).
 *   spcor:   the normalised correlation coefficient, always float, in the reference's doubles and in its order; +0 where
 *            the ref or the window is constant.
 * Bit-identical to the reference.  Complex images are refused, and a ref wider or taller than
 * VIPS_HIP_CORRELATION_MAX_SIDE pels (whatever the format and the band count): what the kernels' LDS tile and ref
 * table hold. */
#define VIPS_HIP_CORRELATION_MAX_SIDE 64
VIPS_HIP_API int vips_hip_fastcor(VipsHipImage *in, VipsHipImage *ref, VipsHipImage **out);
VIPS_HIP_API int vips_hip_spcor(VipsHipImage *in, VipsHipImage *ref, VipsHipImage **out);
/* The per-band constants of vips_spcor (spcor.c:99-152) of a ref in host memory, after format matching: @pixels holds
 * @height rows of @width pels of @bands elements of @format (non-complex), @stride bytes apart; @out_bands is the band
 * count after band matching (@bands, or anything when @bands is 1: the one band is replicated).  rmean[b] is vips_avg
 * of band b; c1[b] = sqrt(avg((float) (ref - rmean)^2) * N) through vips_linear's float output (its single-constant
 * loop when all means are equal), double for a double ref.  @rmean and @c1 take @out_bands doubles.  No device is
 * needed. */
VIPS_HIP_API int vips_hip_spcor_constants(const void *pixels, int width, int height, int bands, int format, size_t stride,
	int out_bands, double *rmean, double *c1);
/* The kernels' units: 0 / 1 the pels / rows of a block's tile, 2 VIPS_HIP_CORRELATION_MAX_SIDE; 0 for anything else. */
VIPS_HIP_API int vips_hip_correlation_step(int what);

/* ------------------------------------------------ canvas and alpha: embed / gravity / insert / join, flatten, addalpha
 *
 * vips_embed and vips_gravity (conversion/embed.c), vips_insert (insert.c) and vips_join (join.c): exact copies of
 * pels onto a canvas, ONE launch an operation (canvas.hip), any non-complex format, pels of up to 32 bytes.
 * vips_flatten (flatten.c) and vips_addalpha (addalpha.c): any non-complex format and band count (a flatten ink of
 * up to 256 bytes).  Complex images are refused with vips_check_noncomplex's words, "image must be non-complex".
 * Results carry no orientation.
 */
#define VIPS_HIP_CANVAS_MAX_BACKGROUND 32

/* The optional arguments of vips_embed / vips_gravity.  vips_hip_embed_defaults(): extend black, nothing set.
 * @extend_set: the caller gave `extend`; a background without it selects extend background (embed.c:366-368).
 * @n_background 0: not given (the class default, one zero). */
typedef struct {
	int extend; /* VipsHipExtend */
	int extend_set;
	int n_background;
	double background[VIPS_HIP_CANVAS_MAX_BACKGROUND];
} VipsHipEmbed;
VIPS_HIP_API void vips_hip_embed_defaults(VipsHipEmbed *args);

/* The optional arguments of vips_flatten.  Defaults: background 0 (n_background 0: not given), max_alpha from the
 * image's interpretation (flatten.c:454). */
typedef struct {
	int n_background;
	double background[VIPS_HIP_CANVAS_MAX_BACKGROUND];
	int max_alpha_set;
	double max_alpha;
} VipsHipFlatten;
VIPS_HIP_API void vips_hip_flatten_defaults(VipsHipFlatten *args);

/* The optional arguments of vips_insert (expand, background) and vips_join (those, shim and align: a VipsAlign, 0 low,
 * 1 centre, 2 high). */
typedef struct {
	int expand;
	int n_background;
	double background[VIPS_HIP_CANVAS_MAX_BACKGROUND];
	int shim;
	int align;
} VipsHipInsert;
VIPS_HIP_API void vips_hip_insert_defaults(VipsHipInsert *args);

/* VipsCompassDirection, include/vips/conversion.h */
typedef enum {
	VIPS_HIP_COMPASS_CENTRE = 0,
	VIPS_HIP_COMPASS_NORTH,
	VIPS_HIP_COMPASS_EAST,
	VIPS_HIP_COMPASS_SOUTH,
	VIPS_HIP_COMPASS_WEST,
	VIPS_HIP_COMPASS_NORTH_EAST,
	VIPS_HIP_COMPASS_SOUTH_EAST,
	VIPS_HIP_COMPASS_SOUTH_WEST,
	VIPS_HIP_COMPASS_NORTH_WEST,
	VIPS_HIP_COMPASS_LAST
} VipsHipCompassDirection;

/* vips__vector_to_ink (conversion/insert.c:240-363) for an image of @bands elements of @format: element z of the pel is
 * background[n == bands ? z : 0], made a float by vips_linear and cast as vips_cast casts.  Host only.  @ink takes
 * bands * sizeof(format) bytes.  -1 with "linear: vector must have 1 or N elements" for a vector of another length. */
VIPS_HIP_API int vips_hip_vector_to_ink(const double *background, int n, int bands, int format, void *ink);

/* vips_embed_base_build restated (embed.c:345-535): *@mode is 0 when the result is a copy of the input (the identity
 * case), else 1; *@extend the extend mode that runs; @ink (32 bytes) the pel of black / white / background.  Errors in
 * the reference's words after @nickname: "bad dimensions" when the image misses the canvas in black / white /
 * background / copy (repeat and mirror take that case), the vector's length.  white is what vips_region_paint writes
 * (iofuncs/region.c:909-956): (int) vips_interpretation_max_alpha as a memset byte for integer formats, as a value
 * for float and double.  No device is touched. */
VIPS_HIP_API int vips_hip_embed_plan(const char *nickname, const VipsHipEmbed *args, int in_width, int in_height,
	int bands, int format, int interpretation, int x, int y, int width, int height, int *mode, int *extend, void *ink);
/* Where vips_gravity puts the image (embed.c:715-790). */
VIPS_HIP_API int vips_hip_gravity_position(int direction, int in_width, int in_height, int width, int height, int *x, int *y);
/* The rectangle of the input image that the canvas rect (left, top, width, height) draws on, for an image of in_width
 * x in_height at (x, y) under @extend (a VipsHipExtend): the bounding box of the pels read; need[2] or need[3] is 0
 * when the rect is all ink. */
VIPS_HIP_API void vips_hip_embed_need(int extend, int in_width, int in_height, int x, int y, int left, int top, int width,
	int height, int need[4]);
/* Fill @out, a window of the canvas (im_width x im_height its size), from @in, a window of the input image that must
 * hold vips_hip_embed_need() of the rect ("input region too small" otherwise).  @extend and @ink as vips_hip_embed_plan
 * gives them.  Bytes of @out's frame outside the window are not touched.  Both regions' memory must cover height *
 * stride bytes from `data`, the last row included: where strides and `data` are multiples of 4 the streaming kernel
 * reads whole aligned dwords, which can take in up to 3 bytes past a row's last pel -- inside that row's stride, never
 * past it. */
VIPS_HIP_API int vips_hip_embed_gen(int extend, const void *ink, int x, int y, const VipsHipRegion *in,
	const VipsHipRegion *out);
/* vips_flatten's generate (flatten.c:167-419) on a pair of windows of the same position and size: @in has one band
 * more than @out, both of one non-complex format.  @ink: out->bands elements of that format (ignored for @black). */
VIPS_HIP_API int vips_hip_flatten_gen(const VipsHipRegion *in, const VipsHipRegion *out, double max_alpha, int black,
	const void *ink);

/* Whole images.  @args NULL: the defaults. */
VIPS_HIP_API int vips_hip_embed(VipsHipImage *in, VipsHipImage **out, int x, int y, int width, int height,
	const VipsHipEmbed *args);
VIPS_HIP_API int vips_hip_gravity(VipsHipImage *in, VipsHipImage **out, int direction, int width, int height,
	const VipsHipEmbed *args);
/* vips_flatten_build (flatten.c:421-529): a one-band image is a copy; integer images whose max_alpha is below the
 * format's maximum go through double and back (vips_hip_cast); uchar images take the table kernels. */
VIPS_HIP_API int vips_hip_flatten(VipsHipImage *in, VipsHipImage **out, const VipsHipFlatten *args);
/* One more band holding vips_interpretation_max_alpha, cast to the format. */
VIPS_HIP_API int vips_hip_addalpha(VipsHipImage *in, VipsHipImage **out);
/* vips_insert_build (insert.c:365-444): vips__formatalike (the common format of arithmetic.c:76-109, vips_hip_cast)
 * and vips__bandalike (one band against n: the band n times) first, then one launch.  Errors in the reference's
 * words: "images must have the same number of bands, or one must be single-band". */
VIPS_HIP_API int vips_hip_insert(VipsHipImage *main, VipsHipImage *sub, VipsHipImage **out, int x, int y,
	const VipsHipInsert *args);
/* vips_join_build (join.c:92-216): @direction a VipsDirection (0 horizontal, 1 vertical); without expand the cut to
 * the smaller image is part of the same launch. */
VIPS_HIP_API int vips_hip_join(VipsHipImage *in1, VipsHipImage *in2, VipsHipImage **out, int direction,
	const VipsHipInsert *args);
/* 0: the threads of a block of the canvas kernels; 1: the bytes of a group of the streaming kernel for @pel_size
 * (0: that pel size takes the one-pel-a-lane kernel); 2: the most blocks a launch has (a streaming launch's blocks, whose
 * lanes take the other groups in turns; the blocks of a row times the rows in flight of the one-pel-a-lane kernels,
 * which take the other rows in turns) -- for tests that want sizes round them. */
VIPS_HIP_API int vips_hip_canvas_step(int what, int pel_size);

/* ------------------------------------------------ sheets and tiles: arrayjoin, replicate, wrap, grid; zoom, subsample
 *
 * vips_arrayjoin (conversion/arrayjoin.c), vips_replicate (replicate.c), vips_wrap (wrap.c) and vips_grid (grid.c):
 * exact copies of pels into a lattice of cells, ONE launch an operation (cells.hip) that writes every output byte once,
 * any non-complex format, pels of up to 32 bytes.  vips_zoom (zoom.c) and vips_subsample (subsample.c) as whole-image
 * calls over vips_hip_zoom_gen / vips_hip_subsample_gen.  Complex images are refused with "image must be non-complex".
 * Results carry no orientation.
 */

/* The optional arguments of vips_arrayjoin.  @across, @hspacing, @vspacing 0: not given (n images across; the widest
 * and the tallest image).  @halign / @valign: a VipsAlign (0 low, 1 centre, 2 high).  @n_background 0: not given (one
 * zero). */
typedef struct {
	int across;
	int shim;
	int n_background;
	double background[VIPS_HIP_CANVAS_MAX_BACKGROUND];
	int halign, valign;
	int hspacing, vspacing;
} VipsHipArrayjoin;
VIPS_HIP_API void vips_hip_arrayjoin_defaults(VipsHipArrayjoin *args);

/* The geometry of vips_arrayjoin_build (arrayjoin.c:231-355) for @n images of widths[i] x heights[i], on plain ints:
 * the output's size, the images across, rects[4 i ..]: left, top, width, height of image i's rect on the output (wider
 * by the shim except in the last column and row; the last image's reaches the right edge), offsets[2 i ..]: where
 * image i's pel (0, 0) lies in its rect -- negative where the image is larger than the spacing and so is cropped, as
 * the reference's vips_embed crops it.  No device is touched. */
VIPS_HIP_API int vips_hip_arrayjoin_plan(const VipsHipArrayjoin *args, int n, const int *widths, const int *heights,
	int *out_width, int *out_height, int *across, int *rects, int *offsets);
/* vips_arrayjoin_build (arrayjoin.c:182-373): vips__formatalike_vec (vips_hip_cast to the common format), then
 * vips__bandalike_vec with the background's length counted in (a one-band image becomes n bands), then one launch over
 * a table of n descriptors.  Output pel (X, Y) is image min(n - 1, X / (hspacing + shim) + Y / (vspacing + shim) *
 * across)'s (arrayjoin.c:119,145: an incomplete last row is filled from the last image's stretched rect) or the
 * background.  All images must be on one device. */
VIPS_HIP_API int vips_hip_arrayjoin(VipsHipImage **in, int n, VipsHipImage **out, const VipsHipArrayjoin *args);

/* vips_replicate_build (replicate.c:140-180): @across x @down copies, each 1 .. 1000000. */
VIPS_HIP_API int vips_hip_replicate(VipsHipImage *in, VipsHipImage **out, int across, int down);
/* vips_wrap_build (wrap.c:65-103): pel (X, Y) is pel ((X + x') mod width, (Y + y') mod height) with the reference's
 * clock arithmetic for x' and y' (x' is the WIDTH when @x is a positive multiple of it).  @x_set / @y_set 0: the
 * defaults, width / 2 and height / 2. */
VIPS_HIP_API int vips_hip_wrap(VipsHipImage *in, VipsHipImage **out, int x, int y, int x_set, int y_set);
/* vips_grid_build (grid.c:148-183): a strip of across * down tiles of @tile_height rows becomes a grid; "bad grid
 * geometry" when the strip's height is not tile_height * across * down. */
VIPS_HIP_API int vips_hip_grid(VipsHipImage *in, VipsHipImage **out, int tile_height, int across, int down);

/* The rows of the input that an output rect draws on, need[4] = left, top, width, height: the bounding box of the pels
 * read.  On an axis where the rect crosses a period of a replicate that is the image's WHOLE width or height (the box
 * of a wrapped interval is everything).  For a grid it is the rows from the first tile touched to the last one: with
 * more than one tile across, a rect that spans tiles draws on tiles that lie far apart in the strip, so a row of the
 * grid needs (across - 1) * tile_height + 1 rows of it, and every column.  That is the honest answer: a bounding box
 * cannot say less.  @x0, @y0: where the output's pel (0, 0) lies in its period (0 for vips_replicate). */
VIPS_HIP_API void vips_hip_replicate_need(int in_width, int in_height, int x0, int y0, int left, int top, int width,
	int height, int need[4]);
VIPS_HIP_API void vips_hip_grid_need(int in_width, int in_height, int tile_height, int across, int left, int top,
	int width, int height, int need[4]);
/* Fill @out, a window of the output (im_width x im_height its size), from @in, a window of the input image that must
 * hold the need of the rect ("input region too small" otherwise).  Bytes of @out's frame outside the window are not
 * touched.  Both regions' memory must cover height * stride bytes from `data` (see vips_hip_embed_gen).
 * vips_wrap is vips_hip_replicate_gen with the image's Xoffset / Yoffset as @x0 / @y0. */
VIPS_HIP_API int vips_hip_replicate_gen(int x0, int y0, const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_grid_gen(int tile_height, int across, const VipsHipRegion *in, const VipsHipRegion *out);

/* vips_zoom_build (zoom.c:309-353): "zoom factors too large" when a side would pass INT_MAX / 2; factors of 1 are a
 * copy.  vips_subsample_build (subsample.c:193-247): sizes round down, "image has shrunk to nothing"; the reference's
 * `point` picks between two loops that make the same pels, so there is nothing to pass. */
VIPS_HIP_API int vips_hip_zoom(VipsHipImage *in, VipsHipImage **out, int xfac, int yfac);
VIPS_HIP_API int vips_hip_subsample(VipsHipImage *in, VipsHipImage **out, int xfac, int yfac);
/* 0: the threads of a block of the cells kernels; 1: the bytes of a group of the streaming kernel for @pel_size
 * (0: that pel size takes the one-pel-a-lane kernel); 2: the most blocks a launch has (a streaming launch's blocks, whose
 * lanes take the other groups in turns; the blocks of a row times the rows in flight of the one-pel-a-lane kernels,
 * which take the other rows in turns) -- for tests that want sizes round them. */
VIPS_HIP_API int vips_hip_cells_step(int what, int pel_size);

/* ------------------------------------------------ arithmetic: linear / invert / abs, add / subtract / multiply / divide,
 * stats / avg / deviate / min / max
 *
 * The pointwise operations of arithmetic/ (linear.c, invert.c, abs.c, add.c, subtract.c, multiply.c, divide.c) on any
 * non-complex format, ONE launch an operation (arith.hip), bit for bit the reference's arithmetic: multiplies and adds
 * separate, float division correctly rounded.  vips_stats and its single-number siblings (stats.c, avg.c, deviate.c,
 * min.c, max.c) in one read-only pass for uchar, char, ushort, short and float images.  Complex images are refused with
 * vips_check_noncomplex's words.  Results carry no orientation.
 */
#define VIPS_HIP_ARITH_MAX_VECTOR 32

/* The arguments of vips_linear: out = in * a + b, @a and @b vectors of 1 or `bands` elements (a one-band image against
 * n elements makes n bands, linear.c:131-145); @uchar: uchar output.  vips_hip_linear_defaults(): a = 1, b = 0. */
typedef struct {
	int n_a;
	double a[VIPS_HIP_ARITH_MAX_VECTOR];
	int n_b;
	double b[VIPS_HIP_ARITH_MAX_VECTOR];
	int uchar;
} VipsHipLinear;
VIPS_HIP_API void vips_hip_linear_defaults(VipsHipLinear *args);

/* VipsHipArith: the operations vips_hip_arith_format and vips_hip_binary_plan know */
typedef enum {
	VIPS_HIP_ARITH_LINEAR = 0,
	VIPS_HIP_ARITH_INVERT,
	VIPS_HIP_ARITH_ABS,
	VIPS_HIP_ARITH_ADD,
	VIPS_HIP_ARITH_SUBTRACT,
	VIPS_HIP_ARITH_MULTIPLY,
	VIPS_HIP_ARITH_DIVIDE,
	VIPS_HIP_ARITH_ROUND,
	VIPS_HIP_ARITH_SIGN,
	VIPS_HIP_ARITH_CLAMP,
	VIPS_HIP_ARITH_MINPAIR,
	VIPS_HIP_ARITH_MAXPAIR,
	VIPS_HIP_ARITH_REMAINDER,
	VIPS_HIP_ARITH_REMAINDER_CONST,
	VIPS_HIP_ARITH_LAST
} VipsHipArith;

/* VipsOperationRound: the reference's values */
typedef enum {
	VIPS_HIP_ROUND_RINT = 0,
	VIPS_HIP_ROUND_CEIL,
	VIPS_HIP_ROUND_FLOOR,
	VIPS_HIP_ROUND_LAST
} VipsHipRound;

/* The operation's format table (linear.c:425-428, invert.c:166-169, abs.c:188-191, add.c:180-183, subtract.c:176-179,
 * multiply.c:197-200, divide.c:199-202, round.c:157-160, sign.c:162-165, clamp.c:139-142, minpair.c:139-142,
 * maxpair.c:139-142, remainder.c:175-178): the output format for an input (for two images: common) format; -1 for a
 * complex or unknown format or operation.  Host only. */
VIPS_HIP_API int vips_hip_arith_format(int op, int format);
/* vips_linear_build restated (linear.c:121-209): the output's bands and format, whether the reference takes its
 * single-element loops (every element of a and of b equal), and a_ready / b_ready (VIPS_HIP_ARITH_MAX_VECTOR doubles each,
 * either may be NULL).  Errors in the reference's words: "linear: vector must have 1 or N elements".  Host only. */
VIPS_HIP_API int vips_hip_linear_plan(const VipsHipLinear *args, int bands, int format, int *out_bands, int *out_format,
	int *single, double *a_ready, double *b_ready);
/* vips_arithmetic_build's three steps for two images (arithmetic.c:436-505): *@format the common format of
 * vips__formatalike (arithmetic.c:76-109), *@out_format the operation's table applied to it, *@bands and
 * *@interpretation by vips__bandalike (one band against n only: "<nickname>: not one band or N bands" otherwise; the
 * interpretation of the image with the most bands, the left one's when they tie), *@width and *@height by
 * vips__sizealike (the larger of each).  Host only. */
VIPS_HIP_API int vips_hip_binary_plan(int op, int left_width, int left_height, int left_bands, int left_format,
	int left_interpretation, int right_width, int right_height, int right_bands, int right_format,
	int right_interpretation, int *format, int *out_format, int *bands, int *interpretation, int *width, int *height);
/* stats.c:133-171 on a (bands + 1) x 10 matrix whose rows 1 .. bands hold min, max, sum, sum2 and the positions: row 0
 * merged from them, then avg and sd of every row, in the reference's double expressions and order.  Host only. */
VIPS_HIP_API int vips_hip_stats_finish(double *matrix, int bands, long long pels);

/* The generate functions on a pair of windows of the same size.  linear: @out has the bands and format
 * vips_hip_linear_plan gives for @in's; invert, abs: the same bands and format.  Bytes of @out's frame outside the
 * window are not touched.  Where `data` and strides are multiples of 4 on both sides the streaming kernel runs,
 * otherwise (and under VIPS_HIP_NO_ARITH_STREAM) the one-element-a-lane kernel. */
VIPS_HIP_API int vips_hip_linear_gen(const VipsHipLinear *args, const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_invert_gen(const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_abs_gen(const VipsHipRegion *in, const VipsHipRegion *out);

/* Whole images.  @args NULL: the defaults.  abs of an unsigned image is a copy (abs.c:88-90). */
VIPS_HIP_API int vips_hip_linear(VipsHipImage *in, VipsHipImage **out, const VipsHipLinear *args);
VIPS_HIP_API int vips_hip_invert(VipsHipImage *in, VipsHipImage **out);
VIPS_HIP_API int vips_hip_abs(VipsHipImage *in, VipsHipImage **out);
/* Two images: an operand whose format is not the common one goes through vips_hip_cast first; then ONE launch, which
 * indexes a one-band operand by pel and reads zero outside an operand's own rectangle (no bandjoin or embed is made).
 * divide gives 0 where the divisor is 0 (divide.c:130). */
VIPS_HIP_API int vips_hip_add(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out);
VIPS_HIP_API int vips_hip_subtract(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out);
VIPS_HIP_API int vips_hip_multiply(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out);
VIPS_HIP_API int vips_hip_divide(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out);

/* vips_round, vips_sign, vips_clamp, vips_minpair, vips_maxpair, vips_remainder and vips_remainder_const (round.c,
 * sign.c, clamp.c, minpair.c, maxpair.c, remainder.c): further expressions of the same two kernels, planned by
 * vips_hip_binary_plan (two images) and vips_hip_const_plan (constants), bit for bit the reference's values.
 *   round      @round a VipsHipRound: rint / ceil / floor in the image's own type; an integer image is a copy.
 *   sign       char, 1 / 0 / -1; a NaN gives -1.
 *   clamp      VIPS_MAX(min, VIPS_MIN(max, pel)) with double bounds (the reference's defaults: 0 and 1), stored to the
 *              image's format: a fractional bound on an integer image is truncated, a NaN pel comes through.
 *   minpair, maxpair   the smaller / larger of two elements; for float and double fmin / fmax: a NaN loses to a number.
 *   remainder  left % right in the common format, -1 (the format's maximum for unsigned formats) where the divisor is
 *              0; for float and double a - b * floor(a / b) in double with a correctly rounded division.
 *   remainder_const   the same against vips_hip_const_plan's c_int: fractional constants are truncated.
 * Three corners in which the reference's behaviour is undefined are defined here and pinned to nothing:
 *   - INT_MIN % -1 of int images (the reference traps) is 0, as every other value % -1 is;
 *   - a clamp bound outside an integer format's range (the reference's out-of-range conversion) saturates at the
 *     format's limits, so clamp never takes a value out of the interval a format can hold;
 *   - minpair / maxpair of zeros of opposite sign: -0 counts as below +0 in either order (the reference's fmin and
 *     fmax answer by the order of their arguments).
 * The region forms work on a pair of windows of the same size; @out has the format vips_hip_arith_format gives and, for
 * remainder_const, vips_hip_const_plan's bands. */
VIPS_HIP_API int vips_hip_round_gen(int round, const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_sign_gen(const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_clamp_gen(double min, double max, const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_remainder_const_gen(const double *c, int n, const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_round(VipsHipImage *in, VipsHipImage **out, int round);
VIPS_HIP_API int vips_hip_sign(VipsHipImage *in, VipsHipImage **out);
VIPS_HIP_API int vips_hip_clamp(VipsHipImage *in, VipsHipImage **out, double min, double max);
VIPS_HIP_API int vips_hip_remainder_const(VipsHipImage *in, VipsHipImage **out, const double *c, int n);
VIPS_HIP_API int vips_hip_minpair(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out);
VIPS_HIP_API int vips_hip_maxpair(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out);
VIPS_HIP_API int vips_hip_remainder(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out);

/* vips_recomb (conversion/recomb.c): every pel's bands against a matrix, out[v] = sum_u m[v][u] * in[u]: colour
 * matrices, sepia, greyscale by weights, channel mixes.  The sum starts at 0.0 and takes the products in order, in
 * double, multiplies and adds separate; the result is float, double for a double image (the conversion rounds to
 * nearest and overflows to an infinity).  The output has the matrix's height as its bands and everything else of the
 * input's header.  Matrices of up to VIPS_HIP_ARITH_MAX_VECTOR x VIPS_HIP_ARITH_MAX_VECTOR; larger ones are refused by
 * name.  ONE launch (recomb.hip): the streaming kernel for 3 -> 3, 3 -> 1, 1 -> 3, 4 -> 4, 4 -> 3 and 3 -> 4 bands of
 * uchar, ushort or float with rows that start on dwords, otherwise (and under VIPS_HIP_NO_RECOMB_STREAM) the
 * one-pel-a-lane kernel.
 *
 * vips_recomb_build's checks in its order and words (recomb.c:174-185: "image must be non-complex" for the image and
 * for the matrix, "image must one band", "bands in must equal matrix width"), then the size limit; *@out_bands and
 * *@out_format as recomb.c:195-197.  Host only. */
VIPS_HIP_API int vips_hip_recomb_plan(int bands, int format, int mwidth, int mheight, int m_bands, int m_format,
	int *out_bands, int *out_format);
/* The generate function on a pair of windows of the same size; @m: @mheight rows of @mwidth doubles in host memory. */
VIPS_HIP_API int vips_hip_recomb_gen(const double *m, int mwidth, int mheight, const VipsHipRegion *in,
	const VipsHipRegion *out);
/* Whole images.  vips_hip_recomb: @m a one-band image of any real format, turned to doubles as vips_check_matrix turns
 * it; only its pels are read (a few doubles cross the bus). */
VIPS_HIP_API int vips_hip_recomb_matrix(VipsHipImage *in, VipsHipImage **out, const double *m, int mwidth, int mheight);
VIPS_HIP_API int vips_hip_recomb(VipsHipImage *in, VipsHipImage **out, VipsHipImage *m);
/* 0: the threads of a block of the recomb kernels; 1: the most blocks a streaming launch has; 2: the most pels a lane of
 * the streaming kernel takes at a time -- for tests that want sizes round them. */
VIPS_HIP_API int vips_hip_recomb_step(int what);

/* vips_sum (arithmetic/sum.c) and vips_bandrank (conversion/bandrank.c) over an array of 1 .. VIPS_HIP_BANDJOIN_MAX
 * images ("<nickname>: arrays of more than 16 images are outside the HIP path" otherwise), aligned as the reference
 * aligns them: the common format (vips__formatalike_vec; images that are not in it go through vips_hip_cast), one band
 * against n (vips__bandalike_vec; a one-band image is indexed by pel), the largest size (vips__sizealike_vec; an image
 * reads zero outside its own rectangle).  ONE launch (nary.hip): the streaming kernel for images of equal bands and
 * size whose rows start on dwords, otherwise (and under VIPS_HIP_NO_NARY_STREAM) the one-element-a-lane kernel.
 *   sum        accumulated in the output's type, image after image in index order: uint for the unsigned formats (it
 *              wraps), int for the signed ones, float, double.
 *   bandrank   the @index-th smallest of the n values of an element, in the common format; @index -1 is n / 2,
 *              @index >= n "bandrank: index out of range"; one image is a copy.  Index 0 and n - 1 are the reference's
 *              minimum and maximum loops: a NaN in the first image stays, a NaN later never wins.  The other indices
 *              give the reference's value for inputs without NaN.
 *
 * The header of the result for @n images (@rank 0: sum, 1: bandrank): *@format the common format, *@out_format the
 * result's, *@out_bands and *@interpretation by vips__bandalike_vec, the largest *@width and *@height, and *@out_index
 * (may be NULL) the index bandrank uses.  Host only. */
VIPS_HIP_API int vips_hip_nary_plan(int rank, int n, const int *widths, const int *heights, const int *bands,
	const int *formats, const int *interpretations, int index, int *format, int *out_format, int *out_bands,
	int *interpretation, int *width, int *height, int *out_index);
VIPS_HIP_API int vips_hip_sum(VipsHipImage **in, int n, VipsHipImage **out);
VIPS_HIP_API int vips_hip_bandrank(VipsHipImage **in, int n, VipsHipImage **out, int index);
/* 0: the threads of a block of the n-ary kernels; 1: the most blocks a launch has (a streaming launch's blocks, the
 * blocks of a row times the rows in flight of the one-element-a-lane kernel); 2: the bytes of the output a lane of the
 * streaming kernel makes at a time for sum and for bandrank's first and last index; 3 / 4: for bandrank's other indices
 * on formats of up to four bytes / on double -- for tests that want sizes round them. */
VIPS_HIP_API int vips_hip_nary_step(int what);

/* vips_stats: @out takes (bands + 1) * 10 doubles, row 0 over all bands, columns min, max, sum, sum2, avg, sd, xmin,
 * ymin, xmax, ymax (stats.c:91-103).  uchar, char, ushort, short and float images (the square of a 32-bit value does not
 * fit the 64-bit accumulator).  Integer sums are exact 64-bit integers converted once; float sums are doubles added in an
 * order the image's geometry fixes.  NaN enters the sums and neither extreme.  Of equal extremes the first in raster
 * order is reported. */
VIPS_HIP_API int vips_hip_stats(VipsHipImage *in, double *out);
/* avg.c:103-105, deviate.c:114-122, min.c / max.c without `size` and the position arrays: row 0 of the matrix. */
VIPS_HIP_API int vips_hip_avg(VipsHipImage *in, double *out);
VIPS_HIP_API int vips_hip_deviate(VipsHipImage *in, double *out);
VIPS_HIP_API int vips_hip_min(VipsHipImage *in, double *out, int *x, int *y);
VIPS_HIP_API int vips_hip_max(VipsHipImage *in, double *out, int *x, int *y);
/* ... vips_hip_min and vips_hip_max take uint and int images too (their kernels compare in the image's own type): the
 * place of the best match in what vips_hip_fastcor writes is found without leaving the device. */
/* 0: the threads of a block of the arithmetic kernels; 1: the bytes of a group of the streaming kernels (of the output
 * for the pointwise kernels, of one band's share of the input for stats); 2 / 3: the most blocks a pointwise / a stats
 * launch has -- for tests that want sizes round them. */
VIPS_HIP_API int vips_hip_arith_step(int what);

/* ------------------------------------------------ masks: relational / boolean, ifthenelse, the band operations
 *
 * vips_relational / vips_relational_const (arithmetic/relational.c), vips_boolean / vips_boolean_const (boolean.c),
 * vips_ifthenelse with and without `blend` (conversion/ifthenelse.c), vips_bandjoin / vips_bandjoin_const
 * (bandjoin.c), vips_extract_band (extract.c), vips_bandmean (bandmean.c) and vips_bandbool (bandbool.c) on any
 * non-complex format, ONE launch an operation (logic.hip), bit for bit the reference's values, format, bands, size and
 * interpretation.  Complex images are refused with vips_check_noncomplex's words.  Results carry no orientation.
 */
#define VIPS_HIP_LOGIC_MAX_VECTOR 32
#define VIPS_HIP_BANDJOIN_MAX 16

/* VipsOperationRelational, VipsOperationBoolean: the reference's values */
typedef enum {
	VIPS_HIP_RELATIONAL_EQUAL = 0,
	VIPS_HIP_RELATIONAL_NOTEQ,
	VIPS_HIP_RELATIONAL_LESS,
	VIPS_HIP_RELATIONAL_LESSEQ,
	VIPS_HIP_RELATIONAL_MORE,
	VIPS_HIP_RELATIONAL_MOREEQ,
	VIPS_HIP_RELATIONAL_LAST
} VipsHipRelational;
typedef enum {
	VIPS_HIP_BOOLEAN_AND = 0,
	VIPS_HIP_BOOLEAN_OR,
	VIPS_HIP_BOOLEAN_EOR,
	VIPS_HIP_BOOLEAN_LSHIFT,
	VIPS_HIP_BOOLEAN_RSHIFT,
	VIPS_HIP_BOOLEAN_LAST
} VipsHipBoolean;

/* The format tables: @boolean 0 relational.c:214-217 (uchar whatever the input), 1 boolean.c:253-256 and
 * bandbool.c:213-216 (integer formats keep their format, the others give int); -1 for an unknown format.  Host only. */
VIPS_HIP_API int vips_hip_logic_format(int boolean, int format);
/* vips_unary_const_build restated (unaryconst.c:54-120) for @n constants against an image of @bands bands:
 * *@out_bands (a one-band image against n constants makes n bands), c_int / c_double (*@out_bands elements each; either
 * may be NULL) and *@is_int (every constant survives the conversion to int; may be NULL).  Errors in the reference's
 * words after @nickname: "vector must have 1 or N elements".  Host only. */
VIPS_HIP_API int vips_hip_const_plan(const char *nickname, const double *c, int n, int bands, int format, int *out_bands,
	int *is_int, int *c_int, double *c_double);
/* vips_arithmetic_build's three steps for the two-image forms (arithmetic.c:436-505), as vips_hip_binary_plan: the
 * common format, the table applied to it, bands and interpretation by vips__bandalike ("relational: not one band or N
 * bands"), the larger of each size.  Host only. */
VIPS_HIP_API int vips_hip_logic_plan(int boolean, int left_width, int left_height, int left_bands, int left_format,
	int left_interpretation, int right_width, int right_height, int right_bands, int right_format,
	int right_interpretation, int *format, int *out_format, int *bands, int *interpretation, int *width, int *height);
/* vips_ifthenelse_build restated (ifthenelse.c:455-520): bands and sizes matched over all three images, *@format the
 * common format of then and else (the condition goes to uchar), the header the then image's once matched.  Host only. */
VIPS_HIP_API int vips_hip_ifthenelse_plan(int cond_width, int cond_height, int cond_bands, int cond_format,
	int cond_interpretation, int then_width, int then_height, int then_bands, int then_format, int then_interpretation,
	int else_width, int else_height, int else_bands, int else_format, int else_interpretation, int *format, int *bands,
	int *interpretation, int *width, int *height);
/* vips_bandary_build for vips_bandjoin (bandary.c:190-245, bandjoin.c:133-160): the common format of all @n images,
 * the sum of their bands, the largest size, image 0's interpretation.  Host only. */
VIPS_HIP_API int vips_hip_bandjoin_plan(int n, const int *widths, const int *heights, const int *bands, const int *formats,
	int interpretation0, int *format, int *out_bands, int *interpretation, int *width, int *height);

/* The generate functions of the one-image operations on a pair of windows of the same size; @out has the bands and
 * format the operation gives for @in's (extract_band: @out's bands are `n`).  Bytes of @out's frame outside the window
 * are not touched.  Where rows start on dwords the streaming kernels run, otherwise (and under
 * VIPS_HIP_NO_LOGIC_STREAM) the one-element-a-lane kernels. */
VIPS_HIP_API int vips_hip_relational_const_gen(int relational, const double *c, int n, const VipsHipRegion *in,
	const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_boolean_const_gen(int boolean, const double *c, int n, const VipsHipRegion *in,
	const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_bandjoin_const_gen(const double *c, int n, const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_extract_band_gen(int band, const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_bandmean_gen(const VipsHipRegion *in, const VipsHipRegion *out);
VIPS_HIP_API int vips_hip_bandbool_gen(int boolean, const VipsHipRegion *in, const VipsHipRegion *out);

/* Whole images.  Constants: 1 or `bands` of them (a one-band image against n makes n bands).  relational_const compares
 * with int constants when every constant is integral and the image an integer format (on a uint image the constant
 * becomes unsigned), with doubles otherwise; boolean_const truncates its constants to int and works on
 * (unsigned int) pel, so its right shift is logical. */
VIPS_HIP_API int vips_hip_relational_const(VipsHipImage *in, VipsHipImage **out, int relational, const double *c, int n);
VIPS_HIP_API int vips_hip_boolean_const(VipsHipImage *in, VipsHipImage **out, int boolean, const double *c, int n);
/* Two images: an operand whose format is not the common one goes through vips_hip_cast first; then ONE launch, which
 * indexes a one-band operand by pel and reads zero outside an operand's own rectangle.  The right shift of signed
 * formats is arithmetic; float and double operands are truncated to int. */
VIPS_HIP_API int vips_hip_relational(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out, int relational);
VIPS_HIP_API int vips_hip_boolean(VipsHipImage *left, VipsHipImage *right, VipsHipImage **out, int boolean);
/* @cond != 0 ? @in1 : @in2, or with @blend (@cond * @in1 + (255 - @cond) * @in2 + 128) / 255 in the reference's int,
 * unsigned or double arithmetic.  A condition that is not uchar goes through vips_hip_cast (which clips), then and else
 * to their common format; then ONE launch.  A one-band condition over operands of any number of bands (a mask over
 * RGB) runs on the streaming kernel too. */
VIPS_HIP_API int vips_hip_ifthenelse(VipsHipImage *cond, VipsHipImage *in1, VipsHipImage *in2, VipsHipImage **out, int blend);
/* 1 .. VIPS_HIP_BANDJOIN_MAX images in ONE launch (one image: a copy). */
VIPS_HIP_API int vips_hip_bandjoin(VipsHipImage **in, int n, VipsHipImage **out);
/* 0 .. VIPS_HIP_BANDJOIN_MAX - 1 constants appended in the image's format, converted as vips__vector_to_pels
 * converts them (through float, then vips_cast: 1.5 -> 1, -300 -> -128 on a char image). */
VIPS_HIP_API int vips_hip_bandjoin_const(VipsHipImage *in, VipsHipImage **out, const double *c, int n);
/* "extract_band: bad extract band" where @band + @n passes the image's bands. */
VIPS_HIP_API int vips_hip_extract_band(VipsHipImage *in, VipsHipImage **out, int band, int n);
VIPS_HIP_API int vips_hip_bandmean(VipsHipImage *in, VipsHipImage **out);
/* and, or, eor; "bandbool: operator lshift not supported across image bands". */
VIPS_HIP_API int vips_hip_bandbool(VipsHipImage *in, VipsHipImage **out, int boolean);
/* 0: the threads of a block of the kernels of logic.hip; 1: the bytes of a group of the streaming kernels; 2: the most
 * blocks a streaming launch has -- for tests that want sizes round them. */
VIPS_HIP_API int vips_hip_logic_step(int what);

/* ------------------------------------------------ trim: project, profile, getpoint, find_trim
 *
 * vips_project with combine sum (arithmetic/project.c), vips_profile (profile.c), vips_getpoint (getpoint.c) and
 * vips_find_trim (find_trim.c) on images in HBM: read-only passes, ONE launch each (trim.hip), identical to the reference
 * in values, format, bands, size and interpretation.  Complex images are refused with vips_check_noncomplex's words
 * (getpoint: they stay outside the path).  combine max and min stay out: COMBINE_PIXELS (project.c:221-248) assigns the
 * first pel a worker thread meets and combines every other one with the zero memset left, so there is no answer to be
 * identical to.
 */
#define VIPS_HIP_TRIM_MAX_BACKGROUND 32

/* vips_project_format_table (project.c:99-102): uchar / ushort / uint -> uint, char / short / int -> int, float /
 * double -> double; -1 for a complex or unknown format.  Host only. */
VIPS_HIP_API int vips_hip_project_format(int format);
/* vips_project_build (project.c:128-178): @columns is width x 1, @rows 1 x height, both with the input's bands, the
 * table's format and interpretation histogram.  Integer sums wrap mod 2^32 as the reference's accumulators do.  Double
 * sums are added in an order the image's geometry fixes (the reference's order depends on when its threads stop,
 * project.c:319-361): the same image gives the same bits on every run.  Images of 1 .. 4 bands whose rows start on dwords
 * take the streaming kernel, everything else (and everything under VIPS_HIP_NO_TRIM_STREAM) one element a lane. */
VIPS_HIP_API int vips_hip_project(VipsHipImage *in, VipsHipImage **columns, VipsHipImage **rows);
/* vips_profile_build (profile.c:113-161): @columns width x 1, for every column and band the y of the first non-zero
 * element or `height`; @rows 1 x height, the x likewise or `width`; both int, interpretation histogram.  Non-zero is C's
 * `if (p[j])` (profile.c:195): a NaN counts, -0.0 does not. */
VIPS_HIP_API int vips_hip_profile(VipsHipImage *in, VipsHipImage **columns, VipsHipImage **rows);
/* vips_getpoint_build (getpoint.c:91-132): the pel at (x, y) as `bands` doubles in @out (@n: its length, at least
 * `bands`).  One copy of the pel, no launch.  "extract_area: bad extract area" for a point outside the image, as
 * vips_crop says it. */
VIPS_HIP_API int vips_hip_getpoint(VipsHipImage *in, int x, int y, double *out, int n);

/* The optional arguments of vips_find_trim (find_trim.c:194-213).  vips_hip_find_trim_defaults(): threshold 10,
 * n_background 0 (not given: vips_interpretation_max_alpha of the image's interpretation, find_trim.c:95-97), line_art
 * off.  A threshold below 0 is not taken, as the reference's property refuses it: the default stays. */
typedef struct {
	double threshold;
	int n_background;
	double background[VIPS_HIP_TRIM_MAX_BACKGROUND];
	int line_art;
} VipsHipFindTrim;
VIPS_HIP_API void vips_hip_find_trim_defaults(VipsHipFindTrim *args);
/* vips_interpretation_max_alpha (iofuncs/header.c:194-206): find_trim's default background.  Host only. */
VIPS_HIP_API double vips_hip_find_trim_background(int interpretation);
/* find_trim.c:145-168 on the two projections of the thresholded image (@columns: `width` sums, @rows: `height`): profile
 * from both ends.  Nothing set gives left = width, top = height, width = height = 0.  Host only. */
VIPS_HIP_API int vips_hip_find_trim_finish(const unsigned int *columns, int width, const unsigned int *rows, int height,
	int *left, int *top, int *out_width, int *out_height);
/* What vips_linear(1, -background), vips_abs and vips_more_const(threshold) (find_trim.c:131-133) make of every byte value
 * of a uchar image of @bands bands: table[band * 256 + value] is 255 or 0, from vips_hip_linear_plan's a_ready / b_ready
 * and single-element rule and the constant as vips_hip_relational_const compares it.  *@fused: the one-launch route
 * takes this image (1 .. 4 bands, a background of 1 or `bands` values); 0 leaves the table alone.  linear's error for
 * a background of another length.  Host only: no kernel runs. */
VIPS_HIP_API int vips_hip_find_trim_table(const VipsHipFindTrim *args, int bands, int interpretation, int *fused,
	unsigned char *table);
/* vips_find_trim_build (find_trim.c:72-171).  Two routes that always agree.  Composed: the reference's chain of this
 * library's own operations -- flatten (an image with alpha), median 3 (unless line_art), linear, abs, more_const, bandor,
 * project -- then ONE copy of the width + height sums and vips_hip_find_trim_finish on the host; what a member refuses,
 * find_trim refuses in that member's words.  Fused: uchar images of 1 .. 4 bands after the flatten with a background of
 * 1 or `bands` values take ONE launch (median, predicate table, bounds) and write nothing the size of the image.
 * VIPS_HIP_NO_TRIM_FUSED forces the composed route.  @args NULL: the defaults. */
VIPS_HIP_API int vips_hip_find_trim(VipsHipImage *in, const VipsHipFindTrim *args, int *left, int *top, int *width,
	int *height);
/* 0: the threads of a block of the kernels of trim.hip; 1: the bytes of a group of the streaming project kernel; 2: the
 * rows of a fused tile; 3: the most blocks a project / profile launch has once it needs more than one row of blocks;
 * 4: the elements of a fused tile's row; 5: the rows a fused block takes; 6: the rows between two meetings of a project
 * block's waves -- for tests that want sizes round them. */
VIPS_HIP_API int vips_hip_trim_step(int what);

/* ------------------------------------------------ regions: labelregions, countlines
 *
 * vips_labelregions (morphology/labelregions.c) and vips_countlines (countlines.c) on images in HBM (regions.hip),
 * identical to the reference in values, format, bands, size and interpretation.
 */

/* vips_labelregions_build (labelregions.c:60-109).  @mask: one band of int, the input's size, interpretation multiband
 * (vips_black cast to int, :76-78): every pel holds the number of its region.  Regions are the 4-connected components
 * of pels that are BYTEWISE equal over the whole pel (draw_flood.c:223-235: +0.0 and -0.0 are two regions, two NaNs with
 * one payload are one), numbered from 1 in raster order of each region's first pel.  *@segments (may be NULL) is the
 * number of regions PLUS ONE: the reference's counter starts at 1 and is stored after the last increment (:86-106).
 * Any real format, pels of up to 32 bytes; complex images, wider pels and images of 2^31 pels and more (a label is an
 * int) are refused by name.  Six launches -- a union-find whose root is a region's smallest linear index, so the
 * numbering is the reference's whatever order the device runs in, the same bits on every run -- and ONE int to the
 * host, when @segments is given.  The planes (an int a pel and 5 / 64 of a byte) come from the pool; there are no
 * strips, since a region can span the image: what does not fit the device's memory is refused with the sizes. */
VIPS_HIP_API int vips_hip_labelregions(VipsHipImage *in, VipsHipImage **mask, int *segments);
/* 0 / 1: the width / height in pels of the tile a block of label_tiles owns; 2: the largest pel in bytes -- for tests
 * that want sizes round them. */
VIPS_HIP_API int vips_hip_labelregions_step(int what);
/* vips_countlines_build (countlines.c:74-121): the reference's chain (moreeq_const 128, a two-tap integer conv with
 * (-1, 1) clipped to uchar, project, avg, / 255) counts RISES -- an element below 128 followed by one at or above 128,
 * down its column for @direction 0 (horizontal), along its row for 1 (vertical); falls do not count and the copied edge
 * makes no transition -- and divides by the extent across the direction times the bands.  The comparison is
 * vips_hip_relational_const's for each format.  ONE read-only launch, ONE 64-bit count to the host, and the reference's
 * divisions in its order on the host.  Any real format and any number of bands; complex images are refused by name, and
 * so are images of more than 2^25 pels along the count (the reference's uint sums could wrap there). */
VIPS_HIP_API int vips_hip_countlines(VipsHipImage *in, int direction, double *nolines);
/* 0: the threads of a block of the countlines kernel (an element a lane); 1: the rows of a block's strip; 2: the most
 * blocks a launch has: the blocks of a row times the strips in flight, the other strips in turns. */
VIPS_HIP_API int vips_hip_countlines_step(int what);

#ifdef __cplusplus
}
#endif

#endif /* VIPS_HIP_H */
