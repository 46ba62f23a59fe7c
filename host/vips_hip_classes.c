/* The class table of the vips-hip module: one GObject subclass of VipsHipOp per *_hip operation -- the original
 * operation's arguments and defaults (libvips/resample, convolution, colour, conversion: each
 * class cites its original) and the hooks the evaluation engine calls (whole-image form, region form for the strip
 * loop).  Textually part of vips_hip_module.c, which holds the engine (device link, base class, host cache, strip
 * producer / ring) and the registration; split out so that neither file has to be read for the other.
 */
/* ------------------------------------------------------------------ subclasses */

#define HIP_SUBCLASS_FULL(TypeName, type_name, nick, desc, STRIP_HOOKS) \
	typedef VipsHipOpClass TypeName##Class; \
	G_DEFINE_TYPE(TypeName, type_name, VIPS_TYPE_HIP_OP); \
	static void type_name##_args(TypeName##Class *class); \
	static void \
	type_name##_class_init(TypeName##Class *class) \
	{ \
		GObjectClass *gobject_class = G_OBJECT_CLASS(class); \
		VipsObjectClass *vobject_class = VIPS_OBJECT_CLASS(class); \
		gobject_class->set_property = vips_object_set_property; \
		gobject_class->get_property = vips_object_get_property; \
		vobject_class->nickname = nick; \
		vobject_class->description = desc; \
		class->compute = type_name##_compute; \
		STRIP_HOOKS \
		type_name##_args(class); \
	}

#define HIP_SUBCLASS(TypeName, type_name, nick, desc) HIP_SUBCLASS_FULL(TypeName, type_name, nick, desc, )

/* For operations with a region form: images over the HBM budget go through in row strips. */
#define HIP_STRIPS(type_name) \
	class->strip_open = type_name##_strip_open; \
	class->strip_need = type_name##_strip_need; \
	class->strip_run = type_name##_strip_run; \
	class->strip_close = type_name##_strip_close;

#define HIP_HALO(type_name) class->halo = type_name##_halo;

/* ---- the region form of the whole resample family
 *
 * vips_reduce / vips_resize / vips_shrink are, per axis, an optional integer box shrink (the
 * `gap` pre-shrink, reduceh.cpp:430-455 / reducev.cpp:894-917, or vips_shrink's own) and an
 * optional residual reduce, vertical axis first (reduce.c:98-121, resize.c:207-228, shrink.c:77-119):
 *     shrinkv(int_v) -> reducev(rv) -> shrinkh(int_h) -> reduceh(rh)
 * Each stage has a generate replacement in the C ABI that works in whole-image coordinates, so a
 * strip of output rows is made by walking its row range back through the vertical stages
 * (vips_hip_reducev_need, x int_v) and the four gens forward, the rows between them on the device.
 */
typedef struct _ResampleStrip {
	/* upsizing (both scales >= 1): vips_resize's scale-only affine (resize.c:230-300), one
	 * generate replacement that works in whole-image coordinates */
	gboolean upsize;
	double hscale, vscale, idx, idy;
	int interpolate;

	int int_v, int_h;
	VipsHipReduce *rv, *rh;
	int w0, h0; /* input */
	int h1;     /* rows after shrinkv */
	int h2;     /* ... after reducev = output rows */
	int w1;     /* columns after shrinkh */
	int w2;     /* ... after reduceh = output columns */
} ResampleStrip;

/* one axis of vips_reduceh_build / vips_reducev_build: the output size, the integer pre-shrink
 * `gap` buys and the residual factor (reduceh.cpp:396-481, reducev.cpp:859-941) */
static int
resample_axis(const char *nick, int in_size, double shrink, VipsKernel kernel, double gap,
	int *int_shrink, int *shrunk_size, VipsHipReduce **reduce, int *out_size)
{
	int size = (int) ((double) in_size / shrink + 0.5);
	double extra = size * shrink - in_size;
	double residual = shrink;

	*int_shrink = 1;
	*shrunk_size = in_size;
	*reduce = NULL;
	if (size <= 0) {
		vips_error(nick, "%s", "image has shrunk to nothing");
		return -1;
	}
	if (gap > 0.0 && kernel != VIPS_KERNEL_NEAREST) {
		const int k = (int) floor((double) in_size / size / gap);

		if (k > 1) {
			*int_shrink = k;
			residual /= k;
			extra /= k;
			*shrunk_size = vips_hip_shrink_out_size(in_size, k, 1); /* "ceil", TRUE */
		}
	}
	*out_size = residual == 1.0 ? *shrunk_size : size;
	if (residual != 1.0 &&
		!(*reduce = vips_hip_reduce_new(kernel, residual, *shrunk_size, size, extra)))
		return hip_fail(nick);

	return 0;
}

static void
resample_strip_close(VipsHipOp *op, void *plan)
{
	ResampleStrip *p = (ResampleStrip *) plan;

	if (p) {
		vips_hip_reduce_free(p->rv);
		vips_hip_reduce_free(p->rh);
		g_free(p);
	}
}

/* vshrink / hshrink >= 1: the factors of the two axes (1 = untouched); int_only: box shrinks of
 * exactly these (integer) factors, rounding up when ceil is set, no reduce */
static int
resample_strip_open(VipsHipOp *op, VipsImage *in, double vshrink, double hshrink, VipsKernel kernel, double gap,
	gboolean int_only, gboolean ceil, void **plan)
{
	const char *nick = VIPS_OBJECT_GET_CLASS(op)->nickname;
	ResampleStrip *p = g_new0(ResampleStrip, 1);

	p->w0 = in->Xsize;
	p->h0 = in->Ysize;
	p->int_v = p->int_h = 1;
	p->h1 = p->h2 = p->h0;
	p->w1 = p->w2 = p->w0;
	if (int_only) {
		p->int_v = (int) vshrink;
		p->int_h = (int) hshrink;
		p->h1 = p->h2 = p->int_v > 1 ? vips_hip_shrink_out_size(p->h0, p->int_v, ceil) : p->h0;
		p->w1 = p->w2 = p->int_h > 1 ? vips_hip_shrink_out_size(p->w0, p->int_h, ceil) : p->w0;
	}
	else if ((vshrink != 1.0 && resample_axis(nick, p->h0, vshrink, kernel, gap, &p->int_v, &p->h1, &p->rv, &p->h2)) ||
		(hshrink != 1.0 && resample_axis(nick, p->w0, hshrink, kernel, gap, &p->int_h, &p->w1, &p->rh, &p->w2))) {
		resample_strip_close(op, p);
		return -1;
	}
	if (p->h2 != op->out->Ysize || p->w2 != op->out->Xsize || p->h1 <= 0 || p->w1 <= 0) {
		/* not the decomposition the original operation's header came from: whole image only */
		resample_strip_close(op, p);
		return 1;
	}
	*plan = p;

	return 0;
}

static void
resample_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	ResampleStrip *p = (ResampleStrip *) plan;
	int top = out_top, rows = out_rows;

	if (p->upsize) {
		/* output row y reads input rows around y / vscale: the bicubic stencil (4 rows) and the
		 * centre-sampling displacement lie well inside a margin of 4 rows either side */
		*in_top = (int) floor(out_top / p->vscale) - 4;
		*in_rows = (int) ceil((out_top + out_rows) / p->vscale) + 4 - *in_top;
		return;
	}
	if (p->rv)
		vips_hip_reducev_need(p->rv, out_top, out_rows, &top, &rows);
	*in_top = top * p->int_v;
	*in_rows = rows * p->int_v;
}

static int
resample_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	ResampleStrip *p = (ResampleStrip *) plan;
	VipsHipImage *tmp[3] = { NULL, NULL, NULL };
	VipsHipRegion cur = *in, next;
	int n = 0, result = 0;
	int top1 = out->top, rows1 = out->height;

	if (p->upsize)
		return vips_hip_upsize_gen(in, out, p->hscale, p->vscale, p->idx, p->idy, p->interpolate, 0)
			? hip_fail(VIPS_OBJECT_GET_CLASS(op)->nickname)
			: 0;
	if (p->rv)
		vips_hip_reducev_need(p->rv, out->top, out->height, &top1, &rows1);

	/* a stage writes into a device image of its own unless it is the last one, which writes `out` */
#define STAGE(LAST, WIDTH, TOP, ROWS, IM_W, IM_H, CALL) \
	do { \
		if (LAST) \
			next = *out; \
		else { \
			if (!(tmp[n] = vips_hip_image_new((WIDTH), (ROWS), in->bands, in->format, 0))) { \
				result = -1; \
				break; \
			} \
			vips_hip_image_region(tmp[n], &next); \
			next.top = (TOP); \
			next.im_width = (IM_W); \
			next.im_height = (IM_H); \
			n++; \
		} \
		if (CALL) \
			result = -1; \
		cur = next; \
	} while (0)

	if (!result && p->int_v > 1)
		STAGE(!p->rv && p->int_h == 1 && !p->rh, p->w0, top1, rows1, p->w0, p->h1,
			vips_hip_shrinkv_gen(p->int_v, &cur, &next));
	/* 16: the fat-strip height the reference's sink evaluates reducev in (thread.c:301-325), what
	 * the whole-image path uses (strips are multiples of 16 lines) */
	if (!result && p->rv)
		STAGE(p->int_h == 1 && !p->rh, p->w0, out->top, out->height, p->w0, p->h2,
			vips_hip_reducev_gen_tiled(p->rv, &cur, &next, 16));
	if (!result && p->int_h > 1)
		STAGE(!p->rh, p->w1, out->top, out->height, p->w1, p->h2, vips_hip_shrinkh_gen(p->int_h, &cur, &next));
	if (!result && p->rh)
		STAGE(TRUE, p->w2, out->top, out->height, p->w2, p->h2, vips_hip_reduceh_gen(p->rh, &cur, &next));
#undef STAGE
	/* (the pool orders reuse of these blocks behind the kernels: same thread, same stream) */
	for (int i = 0; i < 3; i++)
		vips_hip_image_unref(tmp[i]);

	return result ? hip_fail(VIPS_OBJECT_GET_CLASS(op)->nickname) : 0;
}

#define HIP_RESAMPLE_STRIPS(type_name) \
	class->strip_open = type_name##_strip_open; \
	class->strip_need = resample_strip_need; \
	class->strip_run = resample_strip_run; \
	class->strip_close = resample_strip_close;

/* reduce_hip: resample/reduce.c:98-200 */
typedef struct _VipsReduceHip {
	VipsHipOp parent_instance;
	double hshrink, vshrink, gap;
	VipsKernel kernel;
} VipsReduceHip;

static int
vips_reduce_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsReduceHip *reduce = (VipsReduceHip *) op;

	return vips_hip_reduce(in, out, reduce->hshrink, reduce->vshrink, reduce->kernel, reduce->gap);
}

/* The region form (images over the HBM budget): RGBA uchar with an even integer factor and no
 * pre-shrink takes the fused kernel per strip, everything else the chain of generate
 * replacements. */
static int
vips_reduce_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsReduceHip *reduce = (VipsReduceHip *) op;

	if (reduce->kernel == VIPS_KERNEL_NEAREST)
		return 1;
	return resample_strip_open(op, in, reduce->vshrink, reduce->hshrink, reduce->kernel, reduce->gap, FALSE, FALSE,
		plan);
}

static int
vips_reduce_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	ResampleStrip *p = (ResampleStrip *) plan;

	if (p->int_v == 1 && p->int_h == 1 && p->rv && p->rh) {
		const int r = vips_hip_reduce_gen_tiled(p->rv, p->rh, in, out, 16);

		if (r <= 0)
			return r;
	}
	return resample_strip_run(op, plan, in, out);
}

#define VIPS_REDUCE_HIP_STRIPS \
	class->strip_open = vips_reduce_hip_strip_open; \
	class->strip_need = resample_strip_need; \
	class->strip_run = vips_reduce_hip_strip_run; \
	class->strip_close = resample_strip_close;

HIP_SUBCLASS_FULL(VipsReduceHip, vips_reduce_hip, "reduce_hip", "reduce an image (MI355X)",
	VIPS_REDUCE_HIP_STRIPS)

static void
vips_reduce_hip_args(VipsReduceHipClass *class)
{
	VIPS_ARG_DOUBLE(class, "hshrink", 8, "Hshrink", "Horizontal shrink factor",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsReduceHip, hshrink), 1.0, 1000000.0, 1.0);
	VIPS_ARG_DOUBLE(class, "vshrink", 9, "Vshrink", "Vertical shrink factor",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsReduceHip, vshrink), 1.0, 1000000.0, 1.0);
	VIPS_ARG_ENUM(class, "kernel", 3, "Kernel", "Resampling kernel",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsReduceHip, kernel),
		VIPS_TYPE_KERNEL, VIPS_KERNEL_LANCZOS3);
	VIPS_ARG_DOUBLE(class, "gap", 4, "Gap", "Reducing gap",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsReduceHip, gap), 0.0, 1000000.0, 0.0);
}

static void
vips_reduce_hip_init(VipsReduceHip *reduce)
{
	reduce->gap = 0.0;
	reduce->kernel = VIPS_KERNEL_LANCZOS3;
}

/* reduceh_hip / reducev_hip: resample/reduceh.cpp:567-640, reducev.cpp:1077-1150 */
typedef struct _VipsReduce1Hip {
	VipsHipOp parent_instance;
	double shrink, gap;
	VipsKernel kernel;
} VipsReduce1Hip;

typedef VipsReduce1Hip VipsReducehHip;
typedef VipsReduce1Hip VipsReducevHip;

static int
vips_reduceh_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsReduce1Hip *r = (VipsReduce1Hip *) op;

	return vips_hip_reduceh(in, out, r->shrink, r->kernel, r->gap);
}

static int
vips_reducev_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsReduce1Hip *r = (VipsReduce1Hip *) op;

	return vips_hip_reducev(in, out, r->shrink, r->kernel, r->gap);
}

static int
vips_reduceh_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsReduce1Hip *r = (VipsReduce1Hip *) op;

	if (r->kernel == VIPS_KERNEL_NEAREST)
		return 1;
	return resample_strip_open(op, in, 1.0, r->shrink, r->kernel, r->gap, FALSE, FALSE, plan);
}

static int
vips_reducev_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsReduce1Hip *r = (VipsReduce1Hip *) op;

	if (r->kernel == VIPS_KERNEL_NEAREST)
		return 1;
	return resample_strip_open(op, in, r->shrink, 1.0, r->kernel, r->gap, FALSE, FALSE, plan);
}

HIP_SUBCLASS_FULL(VipsReducehHip, vips_reduceh_hip, "reduceh_hip", "shrink an image horizontally (MI355X)",
	HIP_RESAMPLE_STRIPS(vips_reduceh_hip))
HIP_SUBCLASS_FULL(VipsReducevHip, vips_reducev_hip, "reducev_hip", "shrink an image vertically (MI355X)",
	HIP_RESAMPLE_STRIPS(vips_reducev_hip))

#define REDUCE1_ARGS(class, NAME, LONG) \
	VIPS_ARG_DOUBLE(class, NAME, 3, LONG, LONG " shrink factor", \
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsReduce1Hip, shrink), 1.0, 1000000.0, 1.0); \
	VIPS_ARG_ENUM(class, "kernel", 4, "Kernel", "Resampling kernel", \
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsReduce1Hip, kernel), \
		VIPS_TYPE_KERNEL, VIPS_KERNEL_LANCZOS3); \
	VIPS_ARG_DOUBLE(class, "gap", 5, "Gap", "Reducing gap", \
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsReduce1Hip, gap), 0.0, 1000000.0, 0.0);

static void
vips_reduceh_hip_args(VipsReducehHipClass *class)
{
	REDUCE1_ARGS(class, "hshrink", "Hshrink")
}

static void
vips_reducev_hip_args(VipsReducevHipClass *class)
{
	REDUCE1_ARGS(class, "vshrink", "Vshrink")
}

static void
vips_reduceh_hip_init(VipsReducehHip *r)
{
	r->gap = 0.0;
	r->kernel = VIPS_KERNEL_LANCZOS3;
}

static void
vips_reducev_hip_init(VipsReducevHip *r)
{
	r->gap = 0.0;
	r->kernel = VIPS_KERNEL_LANCZOS3;
}

/* shrink_hip: resample/shrink.c:77-172 */
typedef struct _VipsShrinkHip {
	VipsHipOp parent_instance;
	double hshrink, vshrink;
	gboolean ceil;
} VipsShrinkHip;

static int
vips_shrink_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsShrinkHip *shrink = (VipsShrinkHip *) op;

	return vips_hip_shrink(in, out, shrink->hshrink, shrink->vshrink, shrink->ceil);
}

/* shrink.c:77-119: integer factors are the two box shrinks; anything else is vips_reducev /
 * vips_reduceh with "gap", 1.0 */
static int
vips_shrink_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsShrinkHip *shrink = (VipsShrinkHip *) op;

	if ((int) shrink->hshrink == shrink->hshrink && (int) shrink->vshrink == shrink->vshrink)
		return resample_strip_open(op, in, shrink->vshrink, shrink->hshrink, VIPS_KERNEL_LANCZOS3, 0.0, TRUE,
			shrink->ceil, plan);
	return resample_strip_open(op, in, shrink->vshrink, shrink->hshrink, VIPS_KERNEL_LANCZOS3, 1.0, FALSE, FALSE,
		plan);
}

HIP_SUBCLASS_FULL(VipsShrinkHip, vips_shrink_hip, "shrink_hip", "shrink an image (MI355X)",
	HIP_RESAMPLE_STRIPS(vips_shrink_hip))

static void
vips_shrink_hip_args(VipsShrinkHipClass *class)
{
	VIPS_ARG_DOUBLE(class, "hshrink", 8, "Hshrink", "Horizontal shrink factor",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsShrinkHip, hshrink), 1.0, 1000000.0, 1.0);
	VIPS_ARG_DOUBLE(class, "vshrink", 9, "Vshrink", "Vertical shrink factor",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsShrinkHip, vshrink), 1.0, 1000000.0, 1.0);
	VIPS_ARG_BOOL(class, "ceil", 10, "Ceil", "Round-up output dimensions",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsShrinkHip, ceil), FALSE);
}

static void
vips_shrink_hip_init(VipsShrinkHip *shrink)
{
}

/* shrinkh_hip / shrinkv_hip: resample/shrinkh.c:442-480, shrinkv.c:622-660 */
typedef struct _VipsShrink1Hip {
	VipsHipOp parent_instance;
	int shrink;
	gboolean ceil;
} VipsShrink1Hip;

typedef VipsShrink1Hip VipsShrinkhHip;
typedef VipsShrink1Hip VipsShrinkvHip;

static int
vips_shrinkh_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsShrink1Hip *s = (VipsShrink1Hip *) op;

	return vips_hip_shrinkh(in, out, s->shrink, s->ceil);
}

static int
vips_shrinkv_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsShrink1Hip *s = (VipsShrink1Hip *) op;

	return vips_hip_shrinkv(in, out, s->shrink, s->ceil);
}

static int
vips_shrinkh_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsShrink1Hip *s = (VipsShrink1Hip *) op;

	return s->shrink == 1 ? 1 : resample_strip_open(op, in, 1.0, s->shrink, VIPS_KERNEL_LANCZOS3, 0.0, TRUE, s->ceil, plan);
}

static int
vips_shrinkv_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsShrink1Hip *s = (VipsShrink1Hip *) op;

	return s->shrink == 1 ? 1 : resample_strip_open(op, in, s->shrink, 1.0, VIPS_KERNEL_LANCZOS3, 0.0, TRUE, s->ceil, plan);
}

HIP_SUBCLASS_FULL(VipsShrinkhHip, vips_shrinkh_hip, "shrinkh_hip", "shrink an image horizontally (MI355X)",
	HIP_RESAMPLE_STRIPS(vips_shrinkh_hip))
HIP_SUBCLASS_FULL(VipsShrinkvHip, vips_shrinkv_hip, "shrinkv_hip", "shrink an image vertically (MI355X)",
	HIP_RESAMPLE_STRIPS(vips_shrinkv_hip))

#define SHRINK1_ARGS(class, NAME, LONG) \
	VIPS_ARG_INT(class, NAME, 8, LONG, LONG " shrink factor", \
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsShrink1Hip, shrink), 1, 1000000, 1); \
	VIPS_ARG_BOOL(class, "ceil", 10, "Ceil", "Round-up output dimensions", \
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsShrink1Hip, ceil), FALSE);

static void
vips_shrinkh_hip_args(VipsShrinkhHipClass *class)
{
	SHRINK1_ARGS(class, "hshrink", "Hshrink")
}

static void
vips_shrinkv_hip_args(VipsShrinkvHipClass *class)
{
	SHRINK1_ARGS(class, "vshrink", "Vshrink")
}

static void
vips_shrinkh_hip_init(VipsShrinkhHip *s)
{
	s->shrink = 1;
}

static void
vips_shrinkv_hip_init(VipsShrinkvHip *s)
{
	s->shrink = 1;
}

/* resize_hip: resample/resize.c:331-420 (downsizing half) */
typedef struct _VipsResizeHip {
	VipsHipOp parent_instance;
	double scale, vscale, gap;
	VipsKernel kernel;
} VipsResizeHip;

static int
vips_resize_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsResizeHip *resize = (VipsResizeHip *) op;
	double vscale = vips_object_argument_isset(VIPS_OBJECT(op), "vscale") ? resize->vscale : -1.0;

	return vips_hip_resize(in, out, resize->scale, vscale, resize->kernel, resize->gap);
}

/* Both halves of vips_resize have a region form: downsizing (resize.c:207-228: vips_reducev then
 * vips_reduceh, each with its `gap` pre-shrink) and upsizing (the scale-only vips_affine,
 * resize.c:230-300); the nearest kernel (vips_subsample, vips_zoom: resize.c:165-203, 257-266) and
 * one axis up with the other down go through whole. */
static int
vips_resize_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsResizeHip *resize = (VipsResizeHip *) op;
	double hscale = resize->scale;
	double vscale = vips_object_argument_isset(VIPS_OBJECT(op), "vscale") ? resize->vscale : resize->scale;

	if (resize->kernel == VIPS_KERNEL_NEAREST || hscale <= 0.0 || vscale <= 0.0)
		return 1;
	if (hscale >= 1.0 && vscale >= 1.0) {
		/* pure upsizing: vips_affine with the matrix (hscale, 0, 0, vscale), centre sampling and
		 * the interpolator the kernel maps to (resize.c:118-133, 268-300) */
		ResampleStrip *p;

		if (hscale == 1.0 && vscale == 1.0)
			return 1;
		p = g_new0(ResampleStrip, 1);
		p->upsize = TRUE;
		p->hscale = hscale;
		p->vscale = vscale;
		p->idx = 0.5 * (1.0 - 1.0 / hscale);
		p->idy = 0.5 * (1.0 - 1.0 / vscale);
		p->interpolate = resize->kernel == VIPS_KERNEL_LINEAR ? 1 : 2; /* bilinear : bicubic */
		if (vips_hip_affine_out_size(in->Xsize, hscale) != op->out->Xsize ||
			vips_hip_affine_out_size(in->Ysize, vscale) != op->out->Ysize) {
			g_free(p);
			return 1;
		}
		*plan = p;
		return 0;
	}
	if (hscale > 1.0 || vscale > 1.0)
		return 1; /* one axis up, one down: whole image */
	/* "Don't let either axis drop below 1 px." (resize.c:197-200) */
	hscale = VIPS_MAX(hscale, 1.0 / in->Xsize);
	vscale = VIPS_MAX(vscale, 1.0 / in->Ysize);
	return resample_strip_open(op, in, 1.0 / vscale, 1.0 / hscale, resize->kernel, resize->gap, FALSE, FALSE, plan);
}

HIP_SUBCLASS_FULL(VipsResizeHip, vips_resize_hip, "resize_hip", "resize an image (MI355X)",
	HIP_RESAMPLE_STRIPS(vips_resize_hip))

static void
vips_resize_hip_args(VipsResizeHipClass *class)
{
	VIPS_ARG_DOUBLE(class, "scale", 113, "Scale factor", "Scale image by this factor",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsResizeHip, scale), 0.0, 10000000.0, 0.0);
	VIPS_ARG_DOUBLE(class, "vscale", 113, "Vertical scale factor", "Vertical scale image by this factor",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsResizeHip, vscale), 0.0, 10000000.0, 0.0);
	VIPS_ARG_ENUM(class, "kernel", 3, "Kernel", "Resampling kernel",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsResizeHip, kernel),
		VIPS_TYPE_KERNEL, VIPS_KERNEL_LANCZOS3);
	VIPS_ARG_DOUBLE(class, "gap", 4, "Gap", "Reducing gap",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsResizeHip, gap), 0.0, 1000000.0, 2.0);
}

static void
vips_resize_hip_init(VipsResizeHip *resize)
{
	resize->gap = 2.0;
	resize->kernel = VIPS_KERNEL_LANCZOS3;
}

/* thumbnail_image_hip: resample/thumbnail.c:1690-1760 (vips_thumbnail_image) */
typedef struct _VipsThumbnailHip {
	VipsHipOp parent_instance;
	int width, height;
	VipsSize size;
	gboolean linear;
	VipsInteresting crop;
	gboolean no_rotate;
} VipsThumbnailHip;

/* A second object on @in's pixels that carries @image's orientation: the device image may be another operation's
 * result (borrowed), so the tag never goes on @in itself. */
static VipsHipImage *
hip_oriented_view(VipsHipImage *in, VipsImage *image)
{
	VipsHipImage *view = NULL;

	if (vips_hip_rot(in, &view, VIPS_ANGLE_D0))
		return NULL;
	if (vips_hip_image_set_orientation(view,
			vips_image_get_typeof(image, VIPS_META_ORIENTATION) ? vips_image_get_orientation(image) : 0)) {
		vips_hip_image_unref(view);
		return NULL;
	}

	return view;
}

static int
vips_thumbnail_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsThumbnailHip *thumbnail = (VipsThumbnailHip *) op;
	int height = vips_object_argument_isset(VIPS_OBJECT(op), "height") ? thumbnail->height : 0;
	VipsHipImage *view;
	int result;

	/* the orientation is the VipsImage's (thumbnail.c:592-599); the original rotates unless told not to */
	if (!(view = hip_oriented_view(in, op->ready)))
		return -1;
	result = vips_hip_thumbnail_image_rotate(view, out, thumbnail->width, height, thumbnail->size,
		thumbnail->linear, thumbnail->crop, thumbnail->no_rotate);
	vips_hip_image_unref(view);

	return result;
}

/* The plain case -- a 3-band uchar sRGB image, not linear, no crop: a resize by the factor
 * vips_thumbnail_calculate_shrink picks (thumbnail.c:413-467) -- has the resize's region form;
 * alpha (premultiply), linear light and crops go through whole. */
static int
vips_thumbnail_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsThumbnailHip *thumbnail = (VipsThumbnailHip *) op;
	const int width = thumbnail->width;
	const int height = vips_object_argument_isset(VIPS_OBJECT(op), "height") ? thumbnail->height : width;
	double hshrink, vshrink;

	if (thumbnail->linear || thumbnail->crop != VIPS_INTERESTING_NONE || in->Bands != 3 ||
		in->BandFmt != VIPS_FORMAT_UCHAR || in->Type != VIPS_INTERPRETATION_sRGB)
		return 1;
	/* a rotation has no strip form (an output strip of a quarter turn is an input column band) */
	if (!thumbnail->no_rotate && vips_image_get_orientation(in) != 1)
		return 1;
	hshrink = (double) in->Xsize / width;
	vshrink = (double) in->Ysize / height;
	if (thumbnail->size != VIPS_SIZE_FORCE) {
		if (!(hshrink < vshrink))
			vshrink = hshrink;
		else
			hshrink = vshrink;
	}
	if (thumbnail->size == VIPS_SIZE_UP || hshrink <= 1.0 || vshrink <= 1.0)
		return 1;
	hshrink = VIPS_MIN(hshrink, in->Xsize);
	vshrink = VIPS_MIN(vshrink, in->Ysize);
	/* (through 1 / scale, as vips_hip_thumbnail_image -> vips_hip_resize computes it) */
	hshrink = 1.0 / (1.0 / hshrink);
	vshrink = 1.0 / (1.0 / vshrink);
	return resample_strip_open(op, in, vshrink, hshrink, VIPS_KERNEL_LANCZOS3, 2.0, FALSE, FALSE, plan);
}

HIP_SUBCLASS_FULL(VipsThumbnailHip, vips_thumbnail_hip, "thumbnail_image_hip",
	"generate thumbnail from image (MI355X)", HIP_RESAMPLE_STRIPS(vips_thumbnail_hip))

/* the rotated result has no orientation (vips_autorot removes it, autorot.c:185) */
static int
vips_thumbnail_hip_build(VipsObject *object)
{
	VipsHipOp *op = (VipsHipOp *) object;

	if (VIPS_OBJECT_CLASS(vips_thumbnail_hip_parent_class)->build(object))
		return -1;
	if (!((VipsThumbnailHip *) object)->no_rotate)
		vips_autorot_remove_angle(op->out);

	return 0;
}

static void
vips_thumbnail_hip_args(VipsThumbnailHipClass *class)
{
	VIPS_OBJECT_CLASS(class)->build = vips_thumbnail_hip_build;
	VIPS_ARG_BOOL(class, "no_rotate", 115, "No rotate", "Don't use orientation tags to rotate image upright",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsThumbnailHip, no_rotate), FALSE);
	VIPS_ARG_INT(class, "width", 3, "Target width", "Size to this width",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsThumbnailHip, width), 1, VIPS_MAX_COORD, 1);
	VIPS_ARG_INT(class, "height", 113, "Target height", "Size to this height",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsThumbnailHip, height), 1, VIPS_MAX_COORD, 1);
	VIPS_ARG_ENUM(class, "size", 114, "Size", "Only upsize, only downsize, or both",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsThumbnailHip, size),
		VIPS_TYPE_SIZE, VIPS_SIZE_BOTH);
	VIPS_ARG_BOOL(class, "linear", 118, "Linear", "Reduce in linear light",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsThumbnailHip, linear), FALSE);
	VIPS_ARG_ENUM(class, "crop", 116, "Crop", "Reduce to fill target rectangle, then crop",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsThumbnailHip, crop),
		VIPS_TYPE_INTERESTING, VIPS_INTERESTING_NONE);
}

static void
vips_thumbnail_hip_init(VipsThumbnailHip *thumbnail)
{
	thumbnail->width = 1;
	thumbnail->height = 1;
	thumbnail->size = VIPS_SIZE_BOTH;
	thumbnail->crop = VIPS_INTERESTING_NONE;
}

/* thumbnail_hip: vips_thumbnail() on a file (resample/thumbnail.c:1130-1330, the
 * VipsThumbnailFile class): JPEG shrink-on-load on the host, everything after it on the
 * device.  No input image, so this one is a VipsOperation of its own; it serves its result
 * the way VipsHipOp does.
 */
typedef struct _VipsThumbnailFileHip {
	VipsOperation parent_instance;

	char *filename;
	VipsImage *out;
	int width, height;
	VipsSize size;
	gboolean linear;
	VipsInteresting crop;
	gboolean no_rotate;

	VipsHipImage *result;
	VipsPel *host;
	GMutex lock;
} VipsThumbnailFileHip;

typedef VipsOperationClass VipsThumbnailFileHipClass;

G_DEFINE_TYPE(VipsThumbnailFileHip, vips_thumbnail_file_hip, VIPS_TYPE_OPERATION);

static int
vips_thumbnail_file_hip_gen(VipsRegion *out_region, void *seq, void *a, void *b, gboolean *stop)
{
	VipsThumbnailFileHip *thumbnail = (VipsThumbnailFileHip *) b;
	VipsRect *r = &out_region->valid;
	VipsImage *out = out_region->im;
	const size_t ps = VIPS_IMAGE_SIZEOF_PEL(out);
	const size_t ls = VIPS_IMAGE_SIZEOF_LINE(out);

	if (vips_image_iskilled(out))
		return -1;

	g_mutex_lock(&thumbnail->lock);
	if (!thumbnail->host) {
		VipsPel *host = VIPS_ARRAY(NULL, ls * out->Ysize, VipsPel);

		if (!host || vips_hip_image_write_to_memory(thumbnail->result, host)) {
			g_mutex_unlock(&thumbnail->lock);
			VIPS_FREE(host);
			return hip_fail("thumbnail_hip");
		}
		thumbnail->host = host;
	}
	g_mutex_unlock(&thumbnail->lock);

	for (int y = 0; y < r->height; y++)
		memcpy(VIPS_REGION_ADDR(out_region, r->left, r->top + y),
			thumbnail->host + (size_t) (r->top + y) * ls + (size_t) r->left * ps,
			(size_t) r->width * ps);

	return 0;
}

static VipsHipImage *
vips_thumbnail_file_hip_device(GObject *producer)
{
	return ((VipsThumbnailFileHip *) producer)->result;
}

static int
vips_thumbnail_file_hip_build(VipsObject *object)
{
	VipsThumbnailFileHip *thumbnail = (VipsThumbnailFileHip *) object;
	int height = vips_object_argument_isset(object, "height") ? thumbnail->height : 0;

	if (VIPS_OBJECT_CLASS(vips_thumbnail_file_hip_parent_class)->build(object))
		return -1;

	if (vips_hip_thumbnail_rotate(thumbnail->filename, &thumbnail->result, thumbnail->width, height,
			thumbnail->size, thumbnail->linear, thumbnail->crop, thumbnail->no_rotate) ||
		vips_hip_synchronize())
		return hip_fail("thumbnail_hip");

	g_object_set(object, "out", vips_image_new(), NULL);
	vips_image_init_fields(thumbnail->out,
		vips_hip_image_get_width(thumbnail->result), vips_hip_image_get_height(thumbnail->result),
		vips_hip_image_get_bands(thumbnail->result),
		(VipsBandFormat) vips_hip_image_get_format(thumbnail->result), VIPS_CODING_NONE,
		(VipsInterpretation) vips_hip_image_get_interpretation(thumbnail->result), 1.0, 1.0);
	/* (with no_rotate the tag stays on the result, as on the original's) */
	if (vips_hip_image_get_orientation(thumbnail->result))
		vips_image_set_int(thumbnail->out, VIPS_META_ORIENTATION, vips_hip_image_get_orientation(thumbnail->result));
	if (vips_image_pipelinev(thumbnail->out, VIPS_DEMAND_STYLE_ANY, NULL) ||
		vips_image_generate(thumbnail->out,
			vips_hip_op_start, vips_thumbnail_file_hip_gen, vips_hip_op_stop, NULL, thumbnail))
		return -1;
	hip_link_attach(thumbnail->out, G_OBJECT(thumbnail), vips_thumbnail_file_hip_device);

	return 0;
}

static void
vips_thumbnail_file_hip_dispose(GObject *gobject)
{
	VipsThumbnailFileHip *thumbnail = (VipsThumbnailFileHip *) gobject;

	VIPS_FREE(thumbnail->host);
	if (thumbnail->result) {
		vips_hip_image_unref(thumbnail->result);
		thumbnail->result = NULL;
	}

	G_OBJECT_CLASS(vips_thumbnail_file_hip_parent_class)->dispose(gobject);
}

static void
vips_thumbnail_file_hip_class_init(VipsThumbnailFileHipClass *class)
{
	GObjectClass *gobject_class = G_OBJECT_CLASS(class);
	VipsObjectClass *vobject_class = VIPS_OBJECT_CLASS(class);

	gobject_class->dispose = vips_thumbnail_file_hip_dispose;
	gobject_class->set_property = vips_object_set_property;
	gobject_class->get_property = vips_object_get_property;

	vobject_class->nickname = "thumbnail_hip";
	vobject_class->description = "generate thumbnail from file (MI355X)";
	vobject_class->build = vips_thumbnail_file_hip_build;

	VIPS_ARG_STRING(class, "filename", 1, "Filename", "Filename to read from",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsThumbnailFileHip, filename), NULL);
	VIPS_ARG_IMAGE(class, "out", 2, "Output", "Output image",
		VIPS_ARGUMENT_REQUIRED_OUTPUT, G_STRUCT_OFFSET(VipsThumbnailFileHip, out));
	VIPS_ARG_INT(class, "width", 3, "Target width", "Size to this width",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsThumbnailFileHip, width), 1, VIPS_MAX_COORD, 1);
	VIPS_ARG_INT(class, "height", 113, "Target height", "Size to this height",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsThumbnailFileHip, height), 1, VIPS_MAX_COORD, 1);
	VIPS_ARG_ENUM(class, "size", 114, "Size", "Only upsize, only downsize, or both",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsThumbnailFileHip, size),
		VIPS_TYPE_SIZE, VIPS_SIZE_BOTH);
	VIPS_ARG_ENUM(class, "crop", 116, "Crop", "Reduce to fill target rectangle, then crop",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsThumbnailFileHip, crop),
		VIPS_TYPE_INTERESTING, VIPS_INTERESTING_NONE);
	VIPS_ARG_BOOL(class, "linear", 118, "Linear", "Reduce in linear light",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsThumbnailFileHip, linear), FALSE);
	VIPS_ARG_BOOL(class, "no_rotate", 115, "No rotate", "Don't use orientation tags to rotate image upright",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsThumbnailFileHip, no_rotate), FALSE);
}

static void
vips_thumbnail_file_hip_init(VipsThumbnailFileHip *thumbnail)
{
	thumbnail->width = 1;
	thumbnail->height = 1;
	thumbnail->size = VIPS_SIZE_BOTH;
	thumbnail->crop = VIPS_INTERESTING_NONE;
	g_mutex_init(&thumbnail->lock);
}

/* a per-pixel operation: a strip reads exactly its own rows */
static int
hip_pointwise_halo(VipsHipOp *op, VipsImage *in, int *above, int *below)
{
	*above = *below = 0;

	return 0;
}

/* conv_hip / convsep_hip: convolution/conv.c:120-175, convsep.c:120-170 */
typedef struct _VipsConvHip {
	VipsHipOp parent_instance;
	VipsImage *mask;
	VipsPrecision precision;
	int layers;
	int cluster;
} VipsConvHip;

typedef VipsConvHip VipsConvsepHip;

static int
vips_conv_hip_run(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out, gboolean separable)
{
	VipsConvHip *conv = (VipsConvHip *) op;
	const char *nick = VIPS_OBJECT_GET_CLASS(op)->nickname;
	VipsImage *M;
	int result;

	if (vips_check_matrix(nick, conv->mask, &M)) {
		vips_hip_error_clear();
		return -1;
	}
	if (separable) {
		if (vips_check_separable(nick, M)) {
			g_object_unref(M);
			return -1;
		}
		/* convsep.c:81-87: approximate goes to vips_convasep with the layers argument */
		if (conv->precision == VIPS_PRECISION_APPROXIMATE)
			result = vips_hip_convasep(in, out, VIPS_MATRIX(M, 0, 0), M->Xsize * M->Ysize,
				vips_image_get_scale(M), vips_image_get_offset(M), conv->layers);
		else
			result = vips_hip_convsep(in, out, VIPS_MATRIX(M, 0, 0), M->Xsize * M->Ysize,
				vips_image_get_scale(M), vips_image_get_offset(M), conv->precision);
	}
	/* conv.c:99-107 */
	else if (conv->precision == VIPS_PRECISION_APPROXIMATE)
		result = vips_hip_conva(in, out, VIPS_MATRIX(M, 0, 0), M->Xsize, M->Ysize,
			vips_image_get_scale(M), vips_image_get_offset(M), conv->layers, conv->cluster);
	else
		result = vips_hip_conv(in, out, VIPS_MATRIX(M, 0, 0), M->Xsize, M->Ysize,
			vips_image_get_scale(M), vips_image_get_offset(M), conv->precision);
	g_object_unref(M);

	return result;
}

static int
vips_conv_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_conv_hip_run(op, in, out, FALSE);
}

static int
vips_convsep_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_conv_hip_run(op, in, out, TRUE);
}

/* The region form of conv_hip (integer and float precision): one plan, vips_hip_conv_gen per
 * strip; a strip reads mask_height / 2 rows above and the rest below (convi.c:778-782). */
typedef struct _ConvStrip {
	VipsHipConv *conv;
	int mask_height;
} ConvStrip;

static void
vips_conv_hip_strip_close(VipsHipOp *op, void *plan)
{
	ConvStrip *p = (ConvStrip *) plan;

	if (p) {
		vips_hip_conv_free(p->conv);
		g_free(p);
	}
}

static int
vips_conv_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsConvHip *conv = (VipsConvHip *) op;
	ConvStrip *p;
	VipsImage *M;

	if (conv->precision == VIPS_PRECISION_APPROXIMATE)
		return 1;
	if (vips_check_matrix("conv_hip", conv->mask, &M))
		return -1;
	p = g_new0(ConvStrip, 1);
	p->mask_height = M->Ysize;
	p->conv = vips_hip_conv_new(VIPS_MATRIX(M, 0, 0), M->Xsize, M->Ysize,
		vips_image_get_scale(M), vips_image_get_offset(M), conv->precision);
	g_object_unref(M);
	if (!p->conv) {
		g_free(p);
		return hip_fail("conv_hip");
	}
	*plan = p;

	return 0;
}

static void
vips_conv_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	const int mask_height = ((ConvStrip *) plan)->mask_height;

	*in_top = out_top - mask_height / 2;
	*in_rows = out_rows + mask_height - 1;
}

static int
vips_conv_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_conv_gen(((ConvStrip *) plan)->conv, in, out);
}

HIP_SUBCLASS_FULL(VipsConvHip, vips_conv_hip, "conv_hip", "convolution operation (MI355X)",
	HIP_STRIPS(vips_conv_hip))
/* convsep.c:61-118: the mask runs along both axes; n taps read n / 2 rows above and the rest
 * below (the same window whatever the precision: the approximate form's box sums included) */
static int
vips_convsep_hip_halo(VipsHipOp *op, VipsImage *in, int *above, int *below)
{
	VipsConvHip *conv = (VipsConvHip *) op;
	VipsImage *M;
	int n;

	if (vips_check_matrix("convsep_hip", conv->mask, &M))
		return -1;
	n = M->Xsize * M->Ysize;
	g_object_unref(M);
	*above = n / 2;
	*below = n - 1 - n / 2;

	return 0;
}

HIP_SUBCLASS_FULL(VipsConvsepHip, vips_convsep_hip, "convsep_hip", "separable convolution operation (MI355X)",
	HIP_HALO(vips_convsep_hip))

#define CONV_ARGS(class) \
	VIPS_ARG_IMAGE(class, "mask", 20, "Mask", "Input matrix image", \
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsConvHip, mask)); \
	VIPS_ARG_ENUM(class, "precision", 103, "Precision", "Convolve with this precision", \
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsConvHip, precision), \
		VIPS_TYPE_PRECISION, VIPS_PRECISION_FLOAT); \
	VIPS_ARG_INT(class, "layers", 104, "Layers", "Use this many layers in approximation", \
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsConvHip, layers), 1, 1000, 5); \
	VIPS_ARG_INT(class, "cluster", 105, "Cluster", "Cluster lines closer than this in approximation", \
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsConvHip, cluster), 1, 100, 1);

static void
vips_conv_hip_args(VipsConvHipClass *class)
{
	CONV_ARGS(class)
}

static void
vips_convsep_hip_args(VipsConvsepHipClass *class)
{
	CONV_ARGS(class)
}

static void
vips_conv_hip_init(VipsConvHip *conv)
{
	conv->precision = VIPS_PRECISION_FLOAT;
	conv->layers = 5;
	conv->cluster = 1;
}

static void
vips_convsep_hip_init(VipsConvsepHip *conv)
{
	conv->precision = VIPS_PRECISION_FLOAT;
	conv->layers = 5;
	conv->cluster = 1;
}

/* gaussblur_hip: convolution/gaussblur.c:118-175 */
typedef struct _VipsGaussblurHip {
	VipsHipOp parent_instance;
	double sigma, min_ampl;
	VipsPrecision precision;
} VipsGaussblurHip;

static int
vips_gaussblur_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsGaussblurHip *g = (VipsGaussblurHip *) op;

	return vips_hip_gaussblur(in, out, g->sigma, g->min_ampl, g->precision);
}

/* gaussblur.c:71-116: vips_gaussmat(sigma, min_ampl, separable, precision) then vips_convsep:
 * the mask's width decides the rows a strip reads */
static int
vips_gaussblur_hip_halo(VipsHipOp *op, VipsImage *in, int *above, int *below)
{
	VipsGaussblurHip *g = (VipsGaussblurHip *) op;
	int n;

	if (g->sigma < 0.2) { /* gaussblur.c:88-92: a copy */
		*above = *below = 0;
		return 0;
	}
	if ((n = vips_hip_gaussmat(g->sigma, g->min_ampl, 1, g->precision, NULL, 0, NULL)) < 0)
		return hip_fail("gaussblur_hip");
	*above = n / 2;
	*below = n - 1 - n / 2;

	return 0;
}

HIP_SUBCLASS_FULL(VipsGaussblurHip, vips_gaussblur_hip, "gaussblur_hip", "gaussian blur (MI355X)",
	HIP_HALO(vips_gaussblur_hip))

static void
vips_gaussblur_hip_args(VipsGaussblurHipClass *class)
{
	VIPS_ARG_DOUBLE(class, "sigma", 3, "Sigma", "Sigma of Gaussian",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsGaussblurHip, sigma), 0.0, 1000, 1.5);
	VIPS_ARG_DOUBLE(class, "min_ampl", 3, "Minimum amplitude", "Minimum amplitude of Gaussian",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsGaussblurHip, min_ampl), 0.001, 1.0, 0.2);
	VIPS_ARG_ENUM(class, "precision", 4, "Precision", "Convolve with this precision",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsGaussblurHip, precision),
		VIPS_TYPE_PRECISION, VIPS_PRECISION_INTEGER);
}

static void
vips_gaussblur_hip_init(VipsGaussblurHip *g)
{
	g->sigma = 1.5;
	g->min_ampl = 0.2;
	g->precision = VIPS_PRECISION_INTEGER;
}

/* sharpen_hip: convolution/sharpen.c:304-395 */
typedef struct _VipsSharpenHip {
	VipsHipOp parent_instance;
	double sigma, x1, y2, y3, m1, m2;
} VipsSharpenHip;

static int
vips_sharpen_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsSharpenHip *s = (VipsSharpenHip *) op;

	return vips_hip_sharpen(in, out, s->sigma, s->x1, s->y2, s->y3, s->m1, s->m2);
}

/* sharpen.c:176-228: everything is per pixel except the blur of L with
 * vips_gaussmat(sigma, 0.1, separable, integer) */
static int
vips_sharpen_hip_halo(VipsHipOp *op, VipsImage *in, int *above, int *below)
{
	VipsSharpenHip *s = (VipsSharpenHip *) op;
	int n;

	if ((n = vips_hip_gaussmat(s->sigma, 0.1, 1, VIPS_PRECISION_INTEGER, NULL, 0, NULL)) < 0)
		return hip_fail("sharpen_hip");
	*above = n / 2;
	*below = n - 1 - n / 2;

	return 0;
}

HIP_SUBCLASS_FULL(VipsSharpenHip, vips_sharpen_hip, "sharpen_hip", "unsharp masking for print (MI355X)",
	HIP_HALO(vips_sharpen_hip))

static void
vips_sharpen_hip_args(VipsSharpenHipClass *class)
{
	VIPS_ARG_DOUBLE(class, "sigma", 3, "Sigma", "Sigma of Gaussian",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsSharpenHip, sigma), 0.000001, 10.0, 0.5);
	VIPS_ARG_DOUBLE(class, "x1", 5, "x1", "Flat/jaggy threshold",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsSharpenHip, x1), 0, 1000000, 2.0);
	VIPS_ARG_DOUBLE(class, "y2", 6, "y2", "Maximum brightening",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsSharpenHip, y2), 0, 1000000, 10.0);
	VIPS_ARG_DOUBLE(class, "y3", 7, "y3", "Maximum darkening",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsSharpenHip, y3), 0, 1000000, 20.0);
	VIPS_ARG_DOUBLE(class, "m1", 8, "m1", "Slope for flat areas",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsSharpenHip, m1), 0, 1000000, 0.0);
	VIPS_ARG_DOUBLE(class, "m2", 9, "m2", "Slope for jaggy areas",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsSharpenHip, m2), 0, 1000000, 3.0);
}

static void
vips_sharpen_hip_init(VipsSharpenHip *s)
{
	s->sigma = 0.5;
	s->x1 = 2.0;
	s->y2 = 10.0;
	s->y3 = 20.0;
	s->m1 = 0.0;
	s->m2 = 3.0;
}

/* colourspace_hip: colour/colourspace.c:614-650 */
typedef struct _VipsColourspaceHip {
	VipsHipOp parent_instance;
	VipsInterpretation space;
} VipsColourspaceHip;

static int
vips_colourspace_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsColourspaceHip *c = (VipsColourspaceHip *) op;

	return vips_hip_colourspace(in, out, c->space);
}

/* gaussblur_hip -> colourspace_hip as one call: vips_hip_gaussblur_colourspace runs both blur
 * passes and the colour route in one kernel on 3-band float images (BASELINE config 3), and
 * the two operations otherwise. */
static int
vips_colourspace_hip_fuse(VipsHipOp *op, VipsHipOp *up, VipsHipImage *up_in, VipsHipImage **out)
{
	VipsColourspaceHip *c = (VipsColourspaceHip *) op;
	VipsGaussblurHip *g;

	if (!G_TYPE_CHECK_INSTANCE_TYPE(up, vips_gaussblur_hip_get_type()))
		return 1;
	g = (VipsGaussblurHip *) up;

	return vips_hip_gaussblur_colourspace(up_in, out, g->sigma, g->min_ampl, g->precision, c->space);
}

HIP_SUBCLASS_FULL(VipsColourspaceHip, vips_colourspace_hip, "colourspace_hip",
	"convert to a new colorspace (MI355X)", class->fuse = vips_colourspace_hip_fuse; class->halo = hip_pointwise_halo;)

static void
vips_colourspace_hip_args(VipsColourspaceHipClass *class)
{
	VIPS_ARG_ENUM(class, "space", 6, "Space", "Destination color space",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsColourspaceHip, space),
		VIPS_TYPE_INTERPRETATION, VIPS_INTERPRETATION_sRGB);
}

static void
vips_colourspace_hip_init(VipsColourspaceHip *c)
{
	c->space = VIPS_INTERPRETATION_sRGB;
}

/* rot_hip / flip_hip / autorot_hip: conversion/rot.c:402-440, flip.c:264-300, autorot.c:193-240.  They evaluate
 * whole -- one device call, the result on the device for a downstream *_hip operation -- and have no strip form:
 * an output strip of a quarter turn is an input column band.  An image over the HBM budget goes to the original
 * operation (hip_wants_original). */
typedef struct _VipsRotHip {
	VipsHipOp parent_instance;
	VipsAngle angle;
} VipsRotHip;

static int
vips_rot_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_hip_rot(in, out, ((VipsRotHip *) op)->angle);
}

HIP_SUBCLASS(VipsRotHip, vips_rot_hip, "rot_hip", "rotate an image (MI355X)")

static void
vips_rot_hip_args(VipsRotHipClass *class)
{
	VIPS_ARG_ENUM(class, "angle", 6, "Angle", "Angle to rotate image",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsRotHip, angle), VIPS_TYPE_ANGLE, VIPS_ANGLE_D90);
}

static void
vips_rot_hip_init(VipsRotHip *rot)
{
	rot->angle = VIPS_ANGLE_D90;
}

typedef struct _VipsFlipHip {
	VipsHipOp parent_instance;
	VipsDirection direction;
} VipsFlipHip;

static int
vips_flip_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_hip_flip(in, out, ((VipsFlipHip *) op)->direction);
}

HIP_SUBCLASS(VipsFlipHip, vips_flip_hip, "flip_hip", "flip an image (MI355X)")

static void
vips_flip_hip_args(VipsFlipHipClass *class)
{
	VIPS_ARG_ENUM(class, "direction", 6, "Direction", "Direction to flip image",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsFlipHip, direction), VIPS_TYPE_DIRECTION,
		VIPS_DIRECTION_HORIZONTAL);
}

static void
vips_flip_hip_init(VipsFlipHip *flip)
{
	flip->direction = VIPS_DIRECTION_HORIZONTAL;
}

typedef struct _VipsAutorotHip {
	VipsHipOp parent_instance;
	VipsAngle angle;
	gboolean flip;
} VipsAutorotHip;

static int
vips_autorot_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsHipImage *view;
	int result;

	if (!(view = hip_oriented_view(in, op->ready)))
		return -1;
	result = vips_hip_autorot(view, out, NULL, NULL);
	vips_hip_image_unref(view);

	return result;
}

HIP_SUBCLASS(VipsAutorotHip, vips_autorot_hip, "autorot_hip", "autorotate image by exif tag (MI355X)")

/* the two outputs are known at build time (autorot.c:119-165), and the result has no orientation (:185) */
static int
vips_autorot_hip_build(VipsObject *object)
{
	static const VipsAngle angles[9] = { VIPS_ANGLE_D0, VIPS_ANGLE_D0, VIPS_ANGLE_D0, VIPS_ANGLE_D180, VIPS_ANGLE_D180,
		VIPS_ANGLE_D90, VIPS_ANGLE_D90, VIPS_ANGLE_D270, VIPS_ANGLE_D270 };
	static const gboolean flips[9] = { FALSE, FALSE, TRUE, FALSE, TRUE, TRUE, FALSE, TRUE, FALSE };
	VipsHipOp *op = (VipsHipOp *) object;
	int orientation;

	if (VIPS_OBJECT_CLASS(vips_autorot_hip_parent_class)->build(object))
		return -1;
	orientation = vips_image_get_orientation(op->in);
	if (orientation < 1 || orientation > 8)
		orientation = 1;
	g_object_set(object, "angle", angles[orientation], "flip", flips[orientation], NULL);
	vips_autorot_remove_angle(op->out);

	return 0;
}

static void
vips_autorot_hip_args(VipsAutorotHipClass *class)
{
	VIPS_OBJECT_CLASS(class)->build = vips_autorot_hip_build;
	VIPS_ARG_ENUM(class, "angle", 6, "Angle", "Angle image was rotated by",
		VIPS_ARGUMENT_OPTIONAL_OUTPUT, G_STRUCT_OFFSET(VipsAutorotHip, angle), VIPS_TYPE_ANGLE, VIPS_ANGLE_D0);
	VIPS_ARG_BOOL(class, "flip", 7, "Flip", "Whether the image was flipped or not",
		VIPS_ARGUMENT_OPTIONAL_OUTPUT, G_STRUCT_OFFSET(VipsAutorotHip, flip), FALSE);
}

static void
vips_autorot_hip_init(VipsAutorotHip *autorot)
{
	autorot->angle = VIPS_ANGLE_D0;
	autorot->flip = FALSE;
}

/* cast_hip: conversion/cast.c:470-520 */
typedef struct _VipsCastHip {
	VipsHipOp parent_instance;
	VipsBandFormat format;
} VipsCastHip;

static int
vips_cast_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsCastHip *c = (VipsCastHip *) op;

	return vips_hip_cast(in, out, c->format);
}

HIP_SUBCLASS_FULL(VipsCastHip, vips_cast_hip, "cast_hip", "cast an image (MI355X)", class->halo = hip_pointwise_halo;)

static void
vips_cast_hip_args(VipsCastHipClass *class)
{
	VIPS_ARG_ENUM(class, "format", 6, "Format", "Format to cast to",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsCastHip, format),
		VIPS_TYPE_BAND_FORMAT, VIPS_FORMAT_UCHAR);
}

static void
vips_cast_hip_init(VipsCastHip *c)
{
	c->format = VIPS_FORMAT_UCHAR;
}

/* premultiply_hip / unpremultiply_hip: conversion/premultiply.c:273-330, unpremultiply.c:340-400 */
typedef struct _VipsPremultiplyHip {
	VipsHipOp parent_instance;
	gboolean uchar;
} VipsPremultiplyHip;

typedef VipsPremultiplyHip VipsUnpremultiplyHip;

static int
vips_premultiply_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_hip_premultiply(in, out, ((VipsPremultiplyHip *) op)->uchar);
}

static int
vips_unpremultiply_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_hip_unpremultiply(in, out, ((VipsPremultiplyHip *) op)->uchar);
}

HIP_SUBCLASS_FULL(VipsPremultiplyHip, vips_premultiply_hip, "premultiply_hip", "premultiply image alpha (MI355X)",
	class->halo = hip_pointwise_halo;)
HIP_SUBCLASS_FULL(VipsUnpremultiplyHip, vips_unpremultiply_hip, "unpremultiply_hip",
	"unpremultiply image alpha (MI355X)", class->halo = hip_pointwise_halo;)

#define PREMUL_ARGS(class) \
	VIPS_ARG_BOOL(class, "uchar", 116, "Uchar", "Use the uchar fast path", \
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsPremultiplyHip, uchar), FALSE);

static void
vips_premultiply_hip_args(VipsPremultiplyHipClass *class)
{
	PREMUL_ARGS(class)
}

static void
vips_unpremultiply_hip_args(VipsUnpremultiplyHipClass *class)
{
	PREMUL_ARGS(class)
}

static void
vips_premultiply_hip_init(VipsPremultiplyHip *p)
{
}

static void
vips_unpremultiply_hip_init(VipsUnpremultiplyHip *p)
{
}

/* rank_hip / morph_hip: morphology/rank.c:541-587, morph.c:943-985.  Both have a region form in the C ABI
 * (vips_hip_rank_gen, vips_hip_morph_gen: the edge copy is by whole-image coordinates), so an image over the HBM
 * budget goes through in row strips; a strip reads the rows vips_hip_rank_need names -- half the window above, the
 * rest below.  The original operation's build has checked the arguments by then (window too large, index out of
 * range, bad mask element: hip_twin_header), in its own words. */
typedef struct _VipsRankHip {
	VipsHipOp parent_instance;
	int width, height, index;
} VipsRankHip;

static int
vips_rank_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsRankHip *rank = (VipsRankHip *) op;

	return vips_hip_rank(in, out, rank->width, rank->height, rank->index);
}

static void
vips_rank_hip_strip_close(VipsHipOp *op, void *plan)
{
}

static int
vips_rank_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	*plan = op; /* (the arguments are the plan) */

	return 0;
}

static void
vips_rank_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	vips_hip_rank_need(((VipsRankHip *) op)->height, out_top, out_rows, in_top, in_rows);
}

static int
vips_rank_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	VipsRankHip *rank = (VipsRankHip *) op;

	return vips_hip_rank_gen(in, out, rank->width, rank->height, rank->index);
}

HIP_SUBCLASS_FULL(VipsRankHip, vips_rank_hip, "rank_hip", "rank filter (MI355X)", HIP_STRIPS(vips_rank_hip))

static void
vips_rank_hip_args(VipsRankHipClass *class)
{
	VIPS_ARG_INT(class, "width", 4, "Width", "Window width in pixels",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsRankHip, width), 1, 100000, 11);
	VIPS_ARG_INT(class, "height", 5, "Height", "Window height in pixels",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsRankHip, height), 1, 100000, 11);
	VIPS_ARG_INT(class, "index", 6, "Index", "Select pixel at index",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsRankHip, index), 0, 100000000, 50);
}

static void
vips_rank_hip_init(VipsRankHip *rank)
{
	rank->width = 11;
	rank->height = 11;
	rank->index = 50;
}

/* hist_local_hip / stdif_hip: histogram/hist_local.c:335-383, stdif.c:322-395.  As rank_hip: a region form in the C ABI
 * (vips_hip_hist_local_gen, vips_hip_stdif_gen: the mirror and the edge copy are by whole-image coordinates), so an
 * image over the HBM budget goes through in row strips that read the rows vips_hip_rank_need names.  "window too
 * large" and "image must be VIPS_FORMAT_UCHAR" are the original's build's, in its own words (hip_twin_header).  (hist_equal has no
 * class here: vips_hist_find works its pixels out in build(), and a build of this module moves no pixels; maplut
 * takes two images and these classes take one.) */
typedef struct _VipsHistLocalHip {
	VipsHipOp parent_instance;
	int width, height, max_slope;
} VipsHistLocalHip;

static int
vips_hist_local_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsHistLocalHip *local = (VipsHistLocalHip *) op;

	return vips_hip_hist_local(in, out, local->width, local->height, local->max_slope);
}

static void
vips_hist_local_hip_strip_close(VipsHipOp *op, void *plan)
{
}

static int
vips_hist_local_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	*plan = op; /* (the arguments are the plan) */

	return 0;
}

static void
vips_hist_local_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	vips_hip_rank_need(((VipsHistLocalHip *) op)->height, out_top, out_rows, in_top, in_rows);
}

static int
vips_hist_local_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	VipsHistLocalHip *local = (VipsHistLocalHip *) op;

	return vips_hip_hist_local_gen(in, out, local->width, local->height, local->max_slope);
}

HIP_SUBCLASS_FULL(VipsHistLocalHip, vips_hist_local_hip, "hist_local_hip", "local histogram equalisation (MI355X)",
	HIP_STRIPS(vips_hist_local_hip))

static void
vips_hist_local_hip_args(VipsHistLocalHipClass *class)
{
	VIPS_ARG_INT(class, "width", 4, "Width", "Window width in pixels",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsHistLocalHip, width), 1, VIPS_MAX_COORD, 1);
	VIPS_ARG_INT(class, "height", 5, "Height", "Window height in pixels",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsHistLocalHip, height), 1, VIPS_MAX_COORD, 1);
	VIPS_ARG_INT(class, "max_slope", 6, "Max slope", "Maximum slope (CLAHE)",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsHistLocalHip, max_slope), 0, 100, 0);
}

static void
vips_hist_local_hip_init(VipsHistLocalHip *local)
{
	local->width = 1;
	local->height = 1;
}

typedef struct _VipsStdifHip {
	VipsHipOp parent_instance;
	int width, height;
	double a, m0, b, s0;
} VipsStdifHip;

static int
vips_stdif_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsStdifHip *stdif = (VipsStdifHip *) op;

	return vips_hip_stdif(in, out, stdif->width, stdif->height, stdif->a, stdif->m0, stdif->b, stdif->s0);
}

static void
vips_stdif_hip_strip_close(VipsHipOp *op, void *plan)
{
}

static int
vips_stdif_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	*plan = op; /* (the arguments are the plan) */

	return 0;
}

static void
vips_stdif_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	vips_hip_rank_need(((VipsStdifHip *) op)->height, out_top, out_rows, in_top, in_rows);
}

static int
vips_stdif_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	VipsStdifHip *stdif = (VipsStdifHip *) op;

	return vips_hip_stdif_gen(in, out, stdif->width, stdif->height, stdif->a, stdif->m0, stdif->b, stdif->s0);
}

HIP_SUBCLASS_FULL(VipsStdifHip, vips_stdif_hip, "stdif_hip", "statistical difference (MI355X)", HIP_STRIPS(vips_stdif_hip))

static void
vips_stdif_hip_args(VipsStdifHipClass *class)
{
	/* (stdif.c:341-395: width and height default to 11 and stop at 256) */
	VIPS_ARG_INT(class, "width", 4, "Width", "Window width in pixels",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsStdifHip, width), 1, 256, 11);
	VIPS_ARG_INT(class, "height", 5, "Height", "Window height in pixels",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsStdifHip, height), 1, 256, 11);
	VIPS_ARG_DOUBLE(class, "a", 2, "Mean weight", "Weight of new mean",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsStdifHip, a), 0.0, 1.0, 0.5);
	VIPS_ARG_DOUBLE(class, "m0", 2, "Mean", "New mean",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsStdifHip, m0), -INFINITY, INFINITY, 128.0);
	VIPS_ARG_DOUBLE(class, "b", 2, "Deviation weight", "Weight of new deviation",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsStdifHip, b), 0.0, 2.0, 0.5);
	VIPS_ARG_DOUBLE(class, "s0", 2, "Deviation", "New deviation",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsStdifHip, s0), -INFINITY, INFINITY, 50.0);
}

static void
vips_stdif_hip_init(VipsStdifHip *stdif)
{
	stdif->width = 11;
	stdif->height = 11;
	stdif->a = 0.5;
	stdif->m0 = 128.0;
	stdif->b = 0.5;
	stdif->s0 = 50.0;
}

typedef struct _VipsMorphHip {
	VipsHipOp parent_instance;
	VipsImage *mask;
	VipsOperationMorphology morph;
} VipsMorphHip;

static int
vips_morph_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsMorphHip *morph = (VipsMorphHip *) op;
	VipsImage *M;
	int result;

	if (vips_check_matrix("morph_hip", morph->mask, &M))
		return -1;
	result = vips_hip_morph(in, out, VIPS_MATRIX(M, 0, 0), M->Xsize, M->Ysize, morph->morph);
	g_object_unref(M);

	return result;
}

static void
vips_morph_hip_strip_close(VipsHipOp *op, void *plan)
{
	VIPS_UNREF(plan);
}

/* the plan is the mask as a matrix image */
static int
vips_morph_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsImage *M;

	if (vips_check_matrix("morph_hip", ((VipsMorphHip *) op)->mask, &M))
		return -1;
	*plan = M;

	return 0;
}

static void
vips_morph_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	vips_hip_rank_need(((VipsImage *) plan)->Ysize, out_top, out_rows, in_top, in_rows);
}

static int
vips_morph_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	VipsImage *M = (VipsImage *) plan;

	return vips_hip_morph_gen(in, out, VIPS_MATRIX(M, 0, 0), M->Xsize, M->Ysize, ((VipsMorphHip *) op)->morph);
}

HIP_SUBCLASS_FULL(VipsMorphHip, vips_morph_hip, "morph_hip", "morphology operation (MI355X)", HIP_STRIPS(vips_morph_hip))

static void
vips_morph_hip_args(VipsMorphHipClass *class)
{
	VIPS_ARG_IMAGE(class, "mask", 20, "Mask", "Input matrix image",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsMorphHip, mask));
	VIPS_ARG_ENUM(class, "morph", 103, "Morphology", "Morphological operation to perform",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsMorphHip, morph),
		VIPS_TYPE_OPERATION_MORPHOLOGY, VIPS_OPERATION_MORPHOLOGY_ERODE);
}

static void
vips_morph_hip_init(VipsMorphHip *morph)
{
	morph->morph = VIPS_OPERATION_MORPHOLOGY_ERODE;
}

/* sobel_hip / scharr_hip / prewitt_hip: convolution/edge.c:205-334.  No arguments beside in and out.  The region form
 * (vips_hip_edge_gen) reads one row above and one below a strip. */
typedef struct _VipsSobelHip {
	VipsHipOp parent_instance;
} VipsSobelHip;
typedef VipsSobelHip VipsScharrHip;
typedef VipsSobelHip VipsPrewittHip;

static int
edge_hip_which(VipsHipOp *op)
{
	const char *nick = VIPS_OBJECT_GET_CLASS(op)->nickname;

	return strcmp(nick, "sobel_hip") == 0 ? VIPS_HIP_EDGE_SOBEL
		: strcmp(nick, "scharr_hip") == 0 ? VIPS_HIP_EDGE_SCHARR
										  : VIPS_HIP_EDGE_PREWITT;
}

static int
vips_sobel_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	switch (edge_hip_which(op)) {
	case VIPS_HIP_EDGE_SOBEL:
		return vips_hip_sobel(in, out);
	case VIPS_HIP_EDGE_SCHARR:
		return vips_hip_scharr(in, out);
	default:
		return vips_hip_prewitt(in, out);
	}
}

static void
vips_sobel_hip_strip_close(VipsHipOp *op, void *plan)
{
}

static int
vips_sobel_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	*plan = op; /* (the class is the plan) */

	return 0;
}

static void
vips_sobel_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	vips_hip_edge_need(out_top, out_rows, in_top, in_rows);
}

static int
vips_sobel_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_edge_gen(in, out, edge_hip_which(op));
}

#define vips_scharr_hip_compute vips_sobel_hip_compute
#define vips_prewitt_hip_compute vips_sobel_hip_compute

HIP_SUBCLASS_FULL(VipsSobelHip, vips_sobel_hip, "sobel_hip", "Sobel edge detector (MI355X)", HIP_STRIPS(vips_sobel_hip))
HIP_SUBCLASS_FULL(VipsScharrHip, vips_scharr_hip, "scharr_hip", "Scharr edge detector (MI355X)", HIP_STRIPS(vips_sobel_hip))
HIP_SUBCLASS_FULL(VipsPrewittHip, vips_prewitt_hip, "prewitt_hip", "Prewitt edge detector (MI355X)",
	HIP_STRIPS(vips_sobel_hip))

static void
vips_sobel_hip_args(VipsSobelHipClass *class)
{
}

static void
vips_scharr_hip_args(VipsScharrHipClass *class)
{
}

static void
vips_prewitt_hip_args(VipsPrewittHipClass *class)
{
}

static void
vips_sobel_hip_init(VipsSobelHip *edge)
{
}

static void
vips_scharr_hip_init(VipsScharrHip *edge)
{
}

static void
vips_prewitt_hip_init(VipsPrewittHip *edge)
{
}

/* compass_hip: convolution/compass.c:149-214.  The original's build has run vips_rot45 on the mask by then (an even or
 * non-square mask fails there, in its words).  The plan of the C ABI is the strip plan; a strip reads half the mask
 * above and the rest below. */
typedef struct _VipsCompassHip {
	VipsHipOp parent_instance;
	VipsImage *mask;
	int times;
	VipsAngle45 angle;
	VipsCombine combine;
	VipsPrecision precision;
	int layers;
	int cluster;
} VipsCompassHip;

typedef struct _CompassStrip {
	VipsHipCompass *plan;
	int size;
} CompassStrip;

static VipsHipCompass *
compass_hip_plan(VipsCompassHip *compass, int *size)
{
	VipsImage *M;
	VipsHipCompass *plan;

	if (vips_check_matrix("compass_hip", compass->mask, &M))
		return NULL;
	plan = vips_hip_compass_new(VIPS_MATRIX(M, 0, 0), M->Xsize, M->Ysize, vips_image_get_scale(M), vips_image_get_offset(M),
		compass->times, compass->angle, compass->combine, compass->precision, compass->layers, compass->cluster);
	if (size)
		*size = M->Ysize;
	g_object_unref(M);

	return plan;
}

static int
vips_compass_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsCompassHip *compass = (VipsCompassHip *) op;
	VipsImage *M;
	int result;

	if (vips_check_matrix("compass_hip", compass->mask, &M))
		return -1;
	result = vips_hip_compass(in, out, VIPS_MATRIX(M, 0, 0), M->Xsize, M->Ysize, vips_image_get_scale(M),
		vips_image_get_offset(M), compass->times, compass->angle, compass->combine, compass->precision, compass->layers,
		compass->cluster);
	g_object_unref(M);

	return result;
}

static void
vips_compass_hip_strip_close(VipsHipOp *op, void *plan)
{
	CompassStrip *p = (CompassStrip *) plan;

	if (p) {
		vips_hip_compass_free(p->plan);
		g_free(p);
	}
}

static int
vips_compass_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	CompassStrip *p = g_new0(CompassStrip, 1);

	if (!(p->plan = compass_hip_plan((VipsCompassHip *) op, &p->size))) {
		g_free(p);
		return hip_fail("compass_hip");
	}
	*plan = p;

	return 0;
}

static void
vips_compass_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	vips_hip_rank_need(((CompassStrip *) plan)->size, out_top, out_rows, in_top, in_rows);
}

static int
vips_compass_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_compass_gen(((CompassStrip *) plan)->plan, in, out);
}

HIP_SUBCLASS_FULL(VipsCompassHip, vips_compass_hip, "compass_hip", "convolve with rotating mask (MI355X)",
	HIP_STRIPS(vips_compass_hip))

static void
vips_compass_hip_args(VipsCompassHipClass *class)
{
	VIPS_ARG_IMAGE(class, "mask", 20, "Mask", "Input matrix image",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsCompassHip, mask));
	VIPS_ARG_INT(class, "times", 101, "Times", "Rotate and convolve this many times",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsCompassHip, times), 1, 1000, 2);
	VIPS_ARG_ENUM(class, "angle", 103, "Angle", "Rotate mask by this much between convolutions",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsCompassHip, angle), VIPS_TYPE_ANGLE45, VIPS_ANGLE45_D90);
	VIPS_ARG_ENUM(class, "combine", 104, "Combine", "Combine convolution results like this",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsCompassHip, combine), VIPS_TYPE_COMBINE, VIPS_COMBINE_MAX);
	VIPS_ARG_ENUM(class, "precision", 203, "Precision", "Convolve with this precision",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsCompassHip, precision), VIPS_TYPE_PRECISION, VIPS_PRECISION_FLOAT);
	VIPS_ARG_INT(class, "layers", 204, "Layers", "Use this many layers in approximation",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsCompassHip, layers), 1, 1000, 5);
	VIPS_ARG_INT(class, "cluster", 205, "Cluster", "Cluster lines closer than this in approximation",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsCompassHip, cluster), 1, 100, 1);
}

static void
vips_compass_hip_init(VipsCompassHip *compass)
{
	compass->times = 2;
	compass->angle = VIPS_ANGLE45_D90;
	compass->combine = VIPS_COMBINE_MAX;
	compass->precision = VIPS_PRECISION_FLOAT;
	compass->layers = 5;
	compass->cluster = 1;
}

/* canny_hip: convolution/canny.c:431-479.  Whole images by vips_hip_canny; above the HBM budget in row strips with a
 * halo: the blur's radius and, for the gradient and the thinning behind it, two rows above and one below, so that what
 * a strip's own edges disturb is cut away. */
typedef struct _VipsCannyHip {
	VipsHipOp parent_instance;
	double sigma;
	VipsPrecision precision;
} VipsCannyHip;

static int
vips_canny_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsCannyHip *canny = (VipsCannyHip *) op;

	return vips_hip_canny(in, out, canny->sigma, canny->precision);
}

static int
vips_canny_hip_halo(VipsHipOp *op, VipsImage *in, int *above, int *below)
{
	VipsCannyHip *canny = (VipsCannyHip *) op;
	int n = 1;

	if (canny->sigma >= 0.2 && /* (gaussblur.c:82: below that the blur is a copy) */
		(n = vips_hip_gaussmat(canny->sigma, 0.2, 1, canny->precision, NULL, 0, NULL)) < 1)
		return hip_fail("canny_hip");
	*above = n / 2 + 2;
	*below = n - 1 - n / 2 + 1;

	return 0;
}

HIP_SUBCLASS_FULL(VipsCannyHip, vips_canny_hip, "canny_hip", "Canny edge detector (MI355X)", HIP_HALO(vips_canny_hip))

static void
vips_canny_hip_args(VipsCannyHipClass *class)
{
	VIPS_ARG_DOUBLE(class, "sigma", 10, "Sigma", "Sigma of Gaussian",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsCannyHip, sigma), 0.01, 1000, 1.4);
	VIPS_ARG_ENUM(class, "precision", 103, "Precision", "Convolve with this precision",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsCannyHip, precision), VIPS_TYPE_PRECISION, VIPS_PRECISION_FLOAT);
}

static void
vips_canny_hip_init(VipsCannyHip *canny)
{
	canny->sigma = 1.4;
	canny->precision = VIPS_PRECISION_FLOAT;
}

/* affine_hip / similarity_hip / rotate_hip: resample/affine.c:627-718, similarity.c:113-300.  One instance struct for
 * the three (similarity and rotate make their matrix, similarity.c:89-92).  The original operation's build has checked
 * the arguments by then and gives the header; the plan of the C ABI (vips_hip_affine_plan_new) restates it without
 * touching a pixel.  In row strips above the HBM budget: a strip's input rows are vips_hip_affine_need of its rect.
 * For an image with alpha that is not premultiplied a strip is the chain premultiply -> affine -> unpremultiply -> cast
 * on its window.
 * What the device refuses -- double and complex images, the other interpolators, pels over 64 bytes -- is the
 * original's (hip_wants_original). */
typedef struct _VipsAffineHip {
	VipsHipOp parent_instance;
	VipsArrayDouble *matrix;
	double scale, angle;
	VipsInterpolate *interpolate;
	VipsArrayInt *oarea;
	double odx, ody, idx, idy;
	VipsArrayDouble *background;
	gboolean premultiplied;
	VipsExtend extend;
} VipsAffineHip;
typedef VipsAffineHip VipsSimilarityHip;
typedef VipsAffineHip VipsRotateHip;

/* -1: an interpolator the device does not have */
static int
affine_hip_interpolator(VipsInterpolate *interpolate)
{
	const char *nick = interpolate ? VIPS_OBJECT_GET_CLASS(interpolate)->nickname : "bilinear";

	return strcmp(nick, "nearest") == 0 ? VIPS_HIP_INTERPOLATE_NEAREST
		: strcmp(nick, "bilinear") == 0 ? VIPS_HIP_INTERPOLATE_BILINEAR
		: strcmp(nick, "bicubic") == 0  ? VIPS_HIP_INTERPOLATE_BICUBIC
										: -1;
}

static int
affine_hip_arguments(VipsHipOp *op, VipsHipAffine *a)
{
	const char *nick = VIPS_OBJECT_GET_CLASS(op)->nickname;
	VipsAffineHip *affine = (VipsAffineHip *) op;

	vips_hip_affine_defaults(a);
	if (strcmp(nick, "affine_hip") == 0) {
		int n;
		const double *m = vips_array_double_get(affine->matrix, &n);

		if (n != 4) {
			vips_error(nick, "%s", "vector must have 4 elements");
			return -1;
		}
		a->a = m[0];
		a->b = m[1];
		a->c = m[2];
		a->d = m[3];
		a->extend = affine->extend;
		a->premultiplied = affine->premultiplied;
		if (vips_object_argument_isset(VIPS_OBJECT(op), "oarea")) {
			const int *r = vips_array_int_get(affine->oarea, &n);

			if (n != 4) {
				vips_error(nick, "%s", "vector must have 4 elements");
				return -1;
			}
			memcpy(a->oarea, r, 4 * sizeof(int));
			a->have_oarea = 1;
		}
	}
	else {
		const double rad = VIPS_RAD(affine->angle);

		a->a = affine->scale * cos(rad);
		a->b = affine->scale * -sin(rad);
		a->c = -a->b;
		a->d = a->a;
	}
	a->interpolate = affine_hip_interpolator(affine->interpolate);
	a->odx = affine->odx;
	a->ody = affine->ody;
	a->idx = affine->idx;
	a->idy = affine->idy;
	if (affine->background) {
		int n;
		const double *v = vips_array_double_get(affine->background, &n);

		if (n > VIPS_HIP_AFFINE_MAX_BACKGROUND) {
			vips_error(nick, "%s", "background too long");
			return -1;
		}
		a->n_background = n;
		memcpy(a->background, v, n * sizeof(double));
	}
	/* the hint of a pipeline is the smallest of its inputs' (iofuncs/image.c): a tiled input makes the affine tiled */
	a->force_tiles = op->ready && op->ready->dhint == VIPS_DEMAND_STYLE_SMALLTILE;

	return 0;
}

static int
vips_affine_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsHipAffine a;

	if (affine_hip_arguments(op, &a))
		return -1;

	return vips_hip_affine(in, out, &a);
}

static void
vips_affine_hip_strip_close(VipsHipOp *op, void *plan)
{
	vips_hip_affine_plan_free((VipsHipAffinePlan *) plan);
}

static int
vips_affine_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsHipAffine a;
	VipsHipAffinePlan *p;

	if (affine_hip_arguments(op, &a))
		return -1;
	if (!(p = vips_hip_affine_plan_new(&a, in->Xsize, in->Ysize, in->Bands, in->BandFmt, in->Type)))
		return hip_fail(VIPS_OBJECT_GET_CLASS(op)->nickname);
	/* the copy has no region form */
	if (vips_hip_affine_plan_get(p, 2)) {
		vips_hip_affine_plan_free(p);
		return 1;
	}
	*plan = p;

	return 0;
}

static void
vips_affine_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	int need[4];

	vips_hip_affine_need((VipsHipAffinePlan *) plan, 0, out_top, op->out->Xsize, out_rows, need);
	/* (a strip of nothing but background reads no row: any one will do) */
	*in_top = need[3] > 0 ? need[1] : 0;
	*in_rows = need[3] > 0 ? need[3] : 1;
}

static int
vips_affine_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	VipsHipAffinePlan *p = (VipsHipAffinePlan *) plan;
	const int tile = vips_hip_affine_plan_get(p, 3);
	const double max_alpha = vips_interpretation_max_alpha(op->ready->Type);
	VipsHipImage *tmp[3] = { NULL, NULL, NULL };
	VipsHipRegion pre, made, un;
	int result = -1;

	if (!vips_hip_affine_plan_get(p, 4))
		return vips_hip_affine_gen(p, in, out, tile);

	/* alpha, not premultiplied (affine.c:546-563, :614-619): the window premultiplied to float, the strip resampled
	 * from that, unpremultiplied and cast back -- three device images that live as long as this call's launches */
	if ((tmp[0] = vips_hip_image_new(in->width, in->height, in->bands, VIPS_HIP_FORMAT_FLOAT, 0)) &&
		(tmp[1] = vips_hip_image_new(out->width, out->height, out->bands, VIPS_HIP_FORMAT_FLOAT, 0)) &&
		(tmp[2] = vips_hip_image_new(out->width, out->height, out->bands, VIPS_HIP_FORMAT_FLOAT, 0))) {
		vips_hip_image_region(tmp[0], &pre);
		pre.left = in->left;
		pre.top = in->top;
		pre.im_width = in->im_width;
		pre.im_height = in->im_height;
		vips_hip_image_region(tmp[1], &made);
		vips_hip_image_region(tmp[2], &un);
		made.left = un.left = out->left;
		made.top = un.top = out->top;
		made.im_width = un.im_width = out->im_width;
		made.im_height = un.im_height = out->im_height;
		if (!vips_hip_premultiply_gen(in, &pre, max_alpha, 0, 0) &&
			!vips_hip_affine_gen(p, &pre, &made, tile) &&
			!vips_hip_premultiply_gen(&made, &un, max_alpha, 0, 1) &&
			!vips_hip_cast_gen(&un, out))
			result = 0;
	}
	for (int i = 0; i < 3; i++)
		if (tmp[i])
			vips_hip_image_unref(tmp[i]);

	return result;
}

#define vips_similarity_hip_compute vips_affine_hip_compute
#define vips_similarity_hip_strip_open vips_affine_hip_strip_open
#define vips_similarity_hip_strip_need vips_affine_hip_strip_need
#define vips_similarity_hip_strip_run vips_affine_hip_strip_run
#define vips_similarity_hip_strip_close vips_affine_hip_strip_close
#define vips_rotate_hip_compute vips_affine_hip_compute
#define vips_rotate_hip_strip_open vips_affine_hip_strip_open
#define vips_rotate_hip_strip_need vips_affine_hip_strip_need
#define vips_rotate_hip_strip_run vips_affine_hip_strip_run
#define vips_rotate_hip_strip_close vips_affine_hip_strip_close

HIP_SUBCLASS_FULL(VipsAffineHip, vips_affine_hip, "affine_hip", "affine transform of an image (MI355X)", HIP_STRIPS(vips_affine_hip))
HIP_SUBCLASS_FULL(VipsSimilarityHip, vips_similarity_hip, "similarity_hip", "similarity transform of an image (MI355X)",
	HIP_STRIPS(vips_similarity_hip))
HIP_SUBCLASS_FULL(VipsRotateHip, vips_rotate_hip, "rotate_hip", "rotate an image by a number of degrees (MI355X)",
	HIP_STRIPS(vips_rotate_hip))

/* what the three share: the interpolator, the background, the four displacements */
static void
affine_hip_common_args(VipsHipOpClass *class, int interpolate_priority, int background_priority)
{
	VIPS_ARG_INTERPOLATE(class, "interpolate", interpolate_priority, "Interpolate", "Interpolate pixels with this",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsAffineHip, interpolate));
	VIPS_ARG_BOXED(class, "background", background_priority, "Background", "Background value",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsAffineHip, background), VIPS_TYPE_ARRAY_DOUBLE);
	VIPS_ARG_DOUBLE(class, "odx", 112, "Output offset", "Horizontal output displacement",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsAffineHip, odx), -10000000, 10000000, 0);
	VIPS_ARG_DOUBLE(class, "ody", 113, "Output offset", "Vertical output displacement",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsAffineHip, ody), -10000000, 10000000, 0);
	VIPS_ARG_DOUBLE(class, "idx", 114, "Input offset", "Horizontal input displacement",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsAffineHip, idx), -10000000, 10000000, 0);
	VIPS_ARG_DOUBLE(class, "idy", 115, "Input offset", "Vertical input displacement",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsAffineHip, idy), -10000000, 10000000, 0);
}

static void
vips_affine_hip_args(VipsAffineHipClass *class)
{
	VIPS_ARG_BOXED(class, "matrix", 110, "Matrix", "Transformation matrix",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsAffineHip, matrix), VIPS_TYPE_ARRAY_DOUBLE);
	affine_hip_common_args(class, 2, 116);
	VIPS_ARG_BOXED(class, "oarea", 111, "Output rect", "Area of output to generate",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsAffineHip, oarea), VIPS_TYPE_ARRAY_INT);
	VIPS_ARG_ENUM(class, "extend", 117, "Extend", "How to generate the extra pixels",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsAffineHip, extend), VIPS_TYPE_EXTEND, VIPS_EXTEND_BACKGROUND);
	VIPS_ARG_BOOL(class, "premultiplied", 117, "Premultiplied", "Images have premultiplied alpha",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsAffineHip, premultiplied), FALSE);
}

static void
vips_similarity_hip_args(VipsSimilarityHipClass *class)
{
	VIPS_ARG_DOUBLE(class, "scale", 3, "Scale", "Scale by this factor",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsAffineHip, scale), 0, 10000000, 1);
	VIPS_ARG_DOUBLE(class, "angle", 4, "Angle", "Rotate clockwise by this many degrees",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsAffineHip, angle), -10000000, 10000000, 0);
	affine_hip_common_args(class, 5, 6);
}

static void
vips_rotate_hip_args(VipsRotateHipClass *class)
{
	VIPS_ARG_DOUBLE(class, "angle", 4, "Angle", "Rotate clockwise by this many degrees",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsAffineHip, angle), -10000000, 10000000, 0);
	affine_hip_common_args(class, 5, 6);
}

static void
vips_affine_hip_init(VipsAffineHip *affine)
{
	affine->scale = 1;
	affine->extend = VIPS_EXTEND_BACKGROUND;
	affine->background = vips_array_double_newv(1, 0.0);
}

static void
vips_similarity_hip_init(VipsSimilarityHip *affine)
{
	vips_affine_hip_init(affine);
}

static void
vips_rotate_hip_init(VipsRotateHip *affine)
{
	vips_affine_hip_init(affine);
}

/* embed_hip / gravity_hip: conversion/embed.c:537-661, :702-860.  The region form (vips_hip_embed_gen) works in
 * whole-canvas coordinates, so an image over the HBM budget goes through in row strips that read the rows
 * vips_hip_embed_need names: for repeat and mirror a strip of border reaches back across the image.  The original's
 * build has checked the arguments by then ("bad dimensions", the vector's length: hip_twin_header), in its own words.
 * (insert and join take two images and these classes take one: they have no class here.) */
typedef struct _VipsEmbedHip {
	VipsHipOp parent_instance;
	int x, y, width, height;
	VipsCompassDirection direction;
	VipsExtend extend;
	VipsArrayDouble *background;
} VipsEmbedHip;

typedef VipsEmbedHip VipsGravityHip;

typedef struct _EmbedStrip {
	int x, y, extend;
	unsigned char ink[32];
} EmbedStrip;

static int
embed_hip_arguments(VipsHipOp *op, VipsHipEmbed *a)
{
	const char *nick = VIPS_OBJECT_GET_CLASS(op)->nickname;
	VipsEmbedHip *embed = (VipsEmbedHip *) op;

	vips_hip_embed_defaults(a);
	a->extend = embed->extend;
	a->extend_set = vips_object_argument_isset(VIPS_OBJECT(op), "extend");
	if (vips_object_argument_isset(VIPS_OBJECT(op), "background") && embed->background) {
		int n;
		const double *v = vips_array_double_get(embed->background, &n);

		if (n > VIPS_HIP_CANVAS_MAX_BACKGROUND) {
			vips_error(nick, "%s", "background too long");
			return -1;
		}
		a->n_background = n;
		memcpy(a->background, v, n * sizeof(double));
	}

	return 0;
}

static int
embed_hip_position(VipsHipOp *op, int in_width, int in_height, int *x, int *y)
{
	VipsEmbedHip *embed = (VipsEmbedHip *) op;

	if (strcmp(VIPS_OBJECT_GET_CLASS(op)->nickname, "gravity_hip") == 0) {
		if (vips_hip_gravity_position(embed->direction, in_width, in_height, embed->width, embed->height, x, y))
			return hip_fail("gravity_hip");
	}
	else {
		*x = embed->x;
		*y = embed->y;
	}

	return 0;
}

static int
vips_embed_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsEmbedHip *embed = (VipsEmbedHip *) op;
	VipsHipEmbed a;

	if (embed_hip_arguments(op, &a))
		return -1;
	if (strcmp(VIPS_OBJECT_GET_CLASS(op)->nickname, "gravity_hip") == 0)
		return vips_hip_gravity(in, out, embed->direction, embed->width, embed->height, &a);

	return vips_hip_embed(in, out, embed->x, embed->y, embed->width, embed->height, &a);
}

static void
vips_embed_hip_strip_close(VipsHipOp *op, void *plan)
{
	g_free(plan);
}

static int
vips_embed_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	const char *nick = VIPS_OBJECT_GET_CLASS(op)->nickname;
	VipsEmbedHip *embed = (VipsEmbedHip *) op;
	VipsHipEmbed a;
	EmbedStrip *p;
	int mode;

	if (embed_hip_arguments(op, &a))
		return -1;
	p = g_new0(EmbedStrip, 1);
	if (embed_hip_position(op, in->Xsize, in->Ysize, &p->x, &p->y) ||
		vips_hip_embed_plan(nick, &a, in->Xsize, in->Ysize, in->Bands, in->BandFmt, in->Type, p->x, p->y,
			embed->width, embed->height, &mode, &p->extend, p->ink)) {
		g_free(p);
		return hip_fail(nick);
	}
	/* the copy has no region form */
	if (!mode) {
		g_free(p);
		return 1;
	}
	*plan = p;

	return 0;
}

static void
vips_embed_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	EmbedStrip *p = (EmbedStrip *) plan;
	int need[4];

	vips_hip_embed_need(p->extend, op->ready->Xsize, op->ready->Ysize, p->x, p->y, 0, out_top, op->out->Xsize, out_rows, need);
	/* (a strip of nothing but ink reads no row: any one will do) */
	*in_top = need[3] > 0 ? need[1] : 0;
	*in_rows = need[3] > 0 ? need[3] : 1;
}

static int
vips_embed_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	EmbedStrip *p = (EmbedStrip *) plan;

	return vips_hip_embed_gen(p->extend, p->ink, p->x, p->y, in, out);
}

#define vips_gravity_hip_compute vips_embed_hip_compute
#define vips_gravity_hip_strip_open vips_embed_hip_strip_open
#define vips_gravity_hip_strip_need vips_embed_hip_strip_need
#define vips_gravity_hip_strip_run vips_embed_hip_strip_run
#define vips_gravity_hip_strip_close vips_embed_hip_strip_close

HIP_SUBCLASS_FULL(VipsEmbedHip, vips_embed_hip, "embed_hip", "embed an image in a larger image (MI355X)", HIP_STRIPS(vips_embed_hip))
HIP_SUBCLASS_FULL(VipsGravityHip, vips_gravity_hip, "gravity_hip", "place an image within a larger image with a certain gravity (MI355X)",
	HIP_STRIPS(vips_gravity_hip))

static void
embed_hip_common_args(VipsHipOpClass *class)
{
	VIPS_ARG_INT(class, "width", 5, "Width", "Image width in pixels",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsEmbedHip, width), 1, 1000000000, 1);
	VIPS_ARG_INT(class, "height", 6, "Height", "Image height in pixels",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsEmbedHip, height), 1, 1000000000, 1);
	VIPS_ARG_ENUM(class, "extend", 7, "Extend", "How to generate the extra pixels",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsEmbedHip, extend), VIPS_TYPE_EXTEND, VIPS_EXTEND_BLACK);
	VIPS_ARG_BOXED(class, "background", 12, "Background", "Color for background pixels",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsEmbedHip, background), VIPS_TYPE_ARRAY_DOUBLE);
}

static void
vips_embed_hip_args(VipsEmbedHipClass *class)
{
	VIPS_ARG_INT(class, "x", 3, "x", "Left edge of input in output",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsEmbedHip, x), -1000000000, 1000000000, 0);
	VIPS_ARG_INT(class, "y", 4, "y", "Top edge of input in output",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsEmbedHip, y), -1000000000, 1000000000, 0);
	embed_hip_common_args(class);
}

static void
vips_gravity_hip_args(VipsGravityHipClass *class)
{
	VIPS_ARG_ENUM(class, "direction", 3, "Direction", "Direction to place image within width/height",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsEmbedHip, direction), VIPS_TYPE_COMPASS_DIRECTION,
		VIPS_COMPASS_DIRECTION_CENTRE);
	embed_hip_common_args(class);
}

static void
vips_embed_hip_init(VipsEmbedHip *embed)
{
	embed->extend = VIPS_EXTEND_BLACK;
	embed->background = vips_array_double_newv(1, 0.0);
}

static void
vips_gravity_hip_init(VipsGravityHip *embed)
{
	vips_embed_hip_init(embed);
}

/* flatten_hip / addalpha_hip: conversion/flatten.c:531-575, addalpha.c:73-99.  Pointwise: an image over the HBM budget
 * goes through in row strips of the same rows.  flatten_hip's strips run the region form, vips_hip_flatten_gen,
 * straight into the strip's output; an integer image whose max_alpha is below its format's range (flatten.c:457-470)
 * is cast to double, flattened and cast back on the strip's window, three region calls.  A one-band image is a copy
 * and has no region form. */
typedef struct _VipsFlattenHip {
	VipsHipOp parent_instance;
	VipsArrayDouble *background;
	double max_alpha;
} VipsFlattenHip;

typedef struct _FlattenStrip {
	double max_alpha;
	int black;
	int through_double;
	unsigned char ink[256];
} FlattenStrip;

static int
flatten_hip_arguments(VipsHipOp *op, VipsHipFlatten *a)
{
	VipsFlattenHip *flatten = (VipsFlattenHip *) op;

	vips_hip_flatten_defaults(a);
	if (flatten->background) {
		int n;
		const double *v = vips_array_double_get(flatten->background, &n);

		if (n > VIPS_HIP_CANVAS_MAX_BACKGROUND) {
			vips_error("flatten_hip", "%s", "background too long");
			return -1;
		}
		a->n_background = n;
		memcpy(a->background, v, n * sizeof(double));
	}
	a->max_alpha_set = vips_object_argument_isset(VIPS_OBJECT(op), "max_alpha");
	a->max_alpha = flatten->max_alpha;

	return 0;
}

static int
vips_flatten_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsHipFlatten a;

	if (flatten_hip_arguments(op, &a))
		return -1;

	return vips_hip_flatten(in, out, &a);
}

static void
vips_flatten_hip_strip_close(VipsHipOp *op, void *plan)
{
	g_free(plan);
}

static int
vips_flatten_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	static const double zero[1] = { 0.0 };
	VipsHipFlatten a;
	FlattenStrip *p;
	const double *bg;
	int n;

	/* the copy has no region form */
	if (in->Bands == 1)
		return 1;
	if (flatten_hip_arguments(op, &a))
		return -1;
	p = g_new0(FlattenStrip, 1);
	p->max_alpha = a.max_alpha_set ? a.max_alpha : vips_interpretation_max_alpha(in->Type);
	p->through_double = vips_band_format_isint(in->BandFmt) && p->max_alpha < vips_image_get_format_max(in->BandFmt);
	n = a.n_background > 0 ? a.n_background : 1;
	bg = a.n_background > 0 ? a.background : zero;
	p->black = 1;
	for (int i = 0; i < n; i++)
		if (bg[i] != 0.0)
			p->black = 0;
	if (!p->black &&
		vips_hip_vector_to_ink(bg, n, in->Bands - 1, p->through_double ? VIPS_HIP_FORMAT_DOUBLE : (int) in->BandFmt, p->ink)) {
		g_free(p);
		return hip_fail("flatten_hip");
	}
	*plan = p;

	return 0;
}

static void
vips_flatten_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	*in_top = out_top;
	*in_rows = out_rows;
}

static int
vips_flatten_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	FlattenStrip *p = (FlattenStrip *) plan;
	VipsHipImage *tmp[2] = { NULL, NULL };
	VipsHipRegion wide, flat;
	int result = -1;

	if (!p->through_double)
		return vips_hip_flatten_gen(in, out, p->max_alpha, p->black, p->ink);

	if ((tmp[0] = vips_hip_image_new(in->width, in->height, in->bands, VIPS_HIP_FORMAT_DOUBLE, 0)) &&
		(tmp[1] = vips_hip_image_new(out->width, out->height, out->bands, VIPS_HIP_FORMAT_DOUBLE, 0))) {
		vips_hip_image_region(tmp[0], &wide);
		wide.left = in->left;
		wide.top = in->top;
		wide.im_width = in->im_width;
		wide.im_height = in->im_height;
		vips_hip_image_region(tmp[1], &flat);
		flat.left = out->left;
		flat.top = out->top;
		flat.im_width = out->im_width;
		flat.im_height = out->im_height;
		if (!vips_hip_cast_gen(in, &wide) &&
			!vips_hip_flatten_gen(&wide, &flat, p->max_alpha, p->black, p->ink) &&
			!vips_hip_cast_gen(&flat, out))
			result = 0;
	}
	for (int i = 0; i < 2; i++)
		if (tmp[i])
			vips_hip_image_unref(tmp[i]);

	return result;
}

HIP_SUBCLASS_FULL(VipsFlattenHip, vips_flatten_hip, "flatten_hip", "flatten alpha out of an image (MI355X)",
	HIP_STRIPS(vips_flatten_hip))

static void
vips_flatten_hip_args(VipsFlattenHipClass *class)
{
	VIPS_ARG_BOXED(class, "background", 2, "Background", "Background value",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsFlattenHip, background), VIPS_TYPE_ARRAY_DOUBLE);
	VIPS_ARG_DOUBLE(class, "max_alpha", 115, "Maximum alpha", "Maximum value of alpha channel",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsFlattenHip, max_alpha), 0, 100000000, 255);
}

static void
vips_flatten_hip_init(VipsFlattenHip *flatten)
{
	flatten->background = vips_array_double_newv(1, 0.0);
	flatten->max_alpha = 255.0;
}

typedef struct _VipsAddAlphaHip {
	VipsHipOp parent_instance;
} VipsAddAlphaHip;

static int
vips_addalpha_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_hip_addalpha(in, out);
}

HIP_SUBCLASS_FULL(VipsAddAlphaHip, vips_addalpha_hip, "addalpha_hip", "append an alpha channel (MI355X)",
	class->halo = hip_pointwise_halo;)

static void
vips_addalpha_hip_args(VipsAddAlphaHipClass *class)
{
}

static void
vips_addalpha_hip_init(VipsAddAlphaHip *addalpha)
{
}

/* linear_hip / invert_hip / abs_hip: arithmetic/linear.c:430-470, invert.c:171-183, abs.c:193-206.  Pointwise: an image
 * over the HBM budget goes through in row strips of the same rows, each strip one call of the region form
 * (vips_hip_linear_gen, vips_hip_invert_gen, vips_hip_abs_gen) straight into the strip's output.  The output's bands
 * and format are the original's (a one-band image against n-element vectors makes n bands; abs of an unsigned image
 * is a copy, which the region form makes too).  Complex images are the original's (hip_wants_original). */
typedef struct _VipsLinearHip {
	VipsHipOp parent_instance;
	VipsArrayDouble *a;
	VipsArrayDouble *b;
	gboolean uchar;
} VipsLinearHip;

static int
linear_hip_arguments(VipsHipOp *op, VipsHipLinear *l)
{
	VipsLinearHip *linear = (VipsLinearHip *) op;
	VipsArrayDouble *vector[2] = { linear->a, linear->b };

	vips_hip_linear_defaults(l);
	for (int i = 0; i < 2; i++) {
		int n;
		const double *v;

		if (!vector[i])
			continue;
		v = vips_array_double_get(vector[i], &n);
		if (n < 1 || n > VIPS_HIP_ARITH_MAX_VECTOR) {
			vips_error("linear_hip", "%s", "vector too long");
			return -1;
		}
		if (i == 0) {
			l->n_a = n;
			memcpy(l->a, v, n * sizeof(double));
		}
		else {
			l->n_b = n;
			memcpy(l->b, v, n * sizeof(double));
		}
	}
	l->uchar = linear->uchar;

	return 0;
}

static int
vips_linear_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsHipLinear l;

	if (linear_hip_arguments(op, &l))
		return -1;

	return vips_hip_linear(in, out, &l);
}

static void
vips_linear_hip_strip_close(VipsHipOp *op, void *plan)
{
	g_free(plan);
}

static int
vips_linear_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsHipLinear *l = g_new0(VipsHipLinear, 1);

	if (linear_hip_arguments(op, l)) {
		g_free(l);
		return -1;
	}
	*plan = l;

	return 0;
}

static void
vips_linear_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	*in_top = out_top;
	*in_rows = out_rows;
}

static int
vips_linear_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_linear_gen((const VipsHipLinear *) plan, in, out);
}

HIP_SUBCLASS_FULL(VipsLinearHip, vips_linear_hip, "linear_hip", "calculate (a * in + b) (MI355X)", HIP_STRIPS(vips_linear_hip))

static void
vips_linear_hip_args(VipsLinearHipClass *class)
{
	VIPS_ARG_BOXED(class, "a", 110, "a", "Multiply by this",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsLinearHip, a), VIPS_TYPE_ARRAY_DOUBLE);
	VIPS_ARG_BOXED(class, "b", 111, "b", "Add this",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsLinearHip, b), VIPS_TYPE_ARRAY_DOUBLE);
	VIPS_ARG_BOOL(class, "uchar", 112, "uchar", "Output should be uchar",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsLinearHip, uchar), FALSE);
}

static void
vips_linear_hip_init(VipsLinearHip *linear)
{
}

typedef struct _VipsInvertHip {
	VipsHipOp parent_instance;
} VipsInvertHip;

typedef VipsInvertHip VipsAbsHip;

static int
vips_invert_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_hip_invert(in, out);
}

static int
vips_abs_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_hip_abs(in, out);
}

/* (no plan: the region forms take nothing but the regions) */
static int
vips_invert_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	*plan = NULL;

	return 0;
}

static void
vips_invert_hip_strip_close(VipsHipOp *op, void *plan)
{
}

static int
vips_invert_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_invert_gen(in, out);
}

static int
vips_abs_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_abs_gen(in, out);
}

#define vips_invert_hip_strip_need vips_linear_hip_strip_need
#define vips_abs_hip_strip_open vips_invert_hip_strip_open
#define vips_abs_hip_strip_need vips_linear_hip_strip_need
#define vips_abs_hip_strip_close vips_invert_hip_strip_close

HIP_SUBCLASS_FULL(VipsInvertHip, vips_invert_hip, "invert_hip", "invert an image (MI355X)", HIP_STRIPS(vips_invert_hip))
HIP_SUBCLASS_FULL(VipsAbsHip, vips_abs_hip, "abs_hip", "absolute value of an image (MI355X)", HIP_STRIPS(vips_abs_hip))

static void
vips_invert_hip_args(VipsInvertHipClass *class)
{
}

static void
vips_invert_hip_init(VipsInvertHip *invert)
{
}

static void
vips_abs_hip_args(VipsAbsHipClass *class)
{
}

static void
vips_abs_hip_init(VipsAbsHip *abs)
{
}

/* round_hip / sign_hip / clamp_hip / remainder_const_hip: arithmetic/round.c:181-190, sign.c:167-179, clamp.c:144-174,
 * remainder.c:360-380.  Pointwise strip classes on the region forms, with the originals' arguments; the output's header
 * is the original's (a one-band image against n constants makes n bands).  Complex images, and more constants than the
 * kernels keep, are the original's (hip_wants_original). */
typedef struct _VipsArith2Hip {
	VipsHipOp parent_instance;
	VipsOperationRound round;
	double min, max;
	VipsArrayDouble *c;
} VipsArith2Hip;

typedef VipsArith2Hip VipsRoundHip;
typedef VipsArith2Hip VipsSignHip;
typedef VipsArith2Hip VipsClampHip;
typedef VipsArith2Hip VipsRemainderConstHip;

static const double *
arith2_hip_constants(VipsHipOp *op, int *n)
{
	VipsArith2Hip *arith = (VipsArith2Hip *) op;

	*n = 0;
	return arith->c ? vips_array_double_get(arith->c, n) : NULL;
}

static int
vips_round_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_hip_round(in, out, ((VipsArith2Hip *) op)->round);
}

static int
vips_sign_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_hip_sign(in, out);
}

static int
vips_clamp_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_hip_clamp(in, out, ((VipsArith2Hip *) op)->min, ((VipsArith2Hip *) op)->max);
}

static int
vips_remainder_const_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	int n;
	const double *c = arith2_hip_constants(op, &n);

	return vips_hip_remainder_const(in, out, c, n);
}

/* (no plan: the region forms take the operation's own arguments) */
static int
vips_round_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_round_gen(((VipsArith2Hip *) op)->round, in, out);
}

static int
vips_sign_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_sign_gen(in, out);
}

static int
vips_clamp_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_clamp_gen(((VipsArith2Hip *) op)->min, ((VipsArith2Hip *) op)->max, in, out);
}

static int
vips_remainder_const_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	int n;
	const double *c = arith2_hip_constants(op, &n);

	return vips_hip_remainder_const_gen(c, n, in, out);
}

#define ARITH2_HIP_STRIPS(type_name) \
	class->strip_open = vips_invert_hip_strip_open; \
	class->strip_need = vips_linear_hip_strip_need; \
	class->strip_run = type_name##_strip_run; \
	class->strip_close = vips_invert_hip_strip_close;

HIP_SUBCLASS_FULL(VipsRoundHip, vips_round_hip, "round_hip", "perform a round function on an image (MI355X)",
	ARITH2_HIP_STRIPS(vips_round_hip))
HIP_SUBCLASS_FULL(VipsSignHip, vips_sign_hip, "sign_hip", "unit vector of pixel (MI355X)", ARITH2_HIP_STRIPS(vips_sign_hip))
HIP_SUBCLASS_FULL(VipsClampHip, vips_clamp_hip, "clamp_hip", "clamp values of an image (MI355X)", ARITH2_HIP_STRIPS(vips_clamp_hip))
HIP_SUBCLASS_FULL(VipsRemainderConstHip, vips_remainder_const_hip, "remainder_const_hip",
	"remainder after integer division of an image and a constant (MI355X)", ARITH2_HIP_STRIPS(vips_remainder_const_hip))

static void
vips_round_hip_args(VipsRoundHipClass *class)
{
	VIPS_ARG_ENUM(class, "round", 200, "Round operation", "Rounding operation to perform",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsArith2Hip, round),
		VIPS_TYPE_OPERATION_ROUND, VIPS_OPERATION_ROUND_RINT);
}

static void
vips_sign_hip_args(VipsSignHipClass *class)
{
}

static void
vips_clamp_hip_args(VipsClampHipClass *class)
{
	VIPS_ARG_DOUBLE(class, "min", 10, "Min", "Minimum value",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsArith2Hip, min), -INFINITY, INFINITY, 0.0);
	VIPS_ARG_DOUBLE(class, "max", 11, "Max", "Maximum value",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsArith2Hip, max), -INFINITY, INFINITY, 1.0);
}

static void
vips_remainder_const_hip_args(VipsRemainderConstHipClass *class)
{
	VIPS_ARG_BOXED(class, "c", 201, "c", "Array of constants",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsArith2Hip, c), VIPS_TYPE_ARRAY_DOUBLE);
}

static void
arith2_hip_init(VipsArith2Hip *arith)
{
	arith->round = VIPS_OPERATION_ROUND_RINT;
	arith->min = 0.0;
	arith->max = 1.0;
}

static void
vips_round_hip_init(VipsRoundHip *arith)
{
	arith2_hip_init(arith);
}

static void
vips_sign_hip_init(VipsSignHip *arith)
{
	arith2_hip_init(arith);
}

static void
vips_clamp_hip_init(VipsClampHip *arith)
{
	arith2_hip_init(arith);
}

static void
vips_remainder_const_hip_init(VipsRemainderConstHip *arith)
{
	arith2_hip_init(arith);
}

/* recomb_hip: conversion/recomb.c:207-240.  The matrix is read where the work starts, as conv_hip reads its mask: a
 * handful of host doubles, not a streamed producer.  Matrices above 32 x 32 are the original's (hip_wants_original). */
typedef struct _VipsRecombHip {
	VipsHipOp parent_instance;
	VipsImage *m;
} VipsRecombHip;

static int
vips_recomb_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsImage *M;
	int result;

	if (vips_check_matrix("recomb_hip", ((VipsRecombHip *) op)->m, &M))
		return -1;
	result = vips_hip_recomb_matrix(in, out, VIPS_MATRIX(M, 0, 0), M->Xsize, M->Ysize);
	g_object_unref(M);

	return result;
}

/* the plan is the matrix as doubles */
static int
vips_recomb_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	VipsImage *M;

	if (vips_check_matrix("recomb_hip", ((VipsRecombHip *) op)->m, &M))
		return -1;
	*plan = M;

	return 0;
}

static int
vips_recomb_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	VipsImage *M = (VipsImage *) plan;

	return vips_hip_recomb_gen(VIPS_MATRIX(M, 0, 0), M->Xsize, M->Ysize, in, out);
}

#define vips_recomb_hip_strip_need vips_linear_hip_strip_need
#define vips_recomb_hip_strip_close vips_morph_hip_strip_close

HIP_SUBCLASS_FULL(VipsRecombHip, vips_recomb_hip, "recomb_hip", "linear recombination with matrix (MI355X)", HIP_STRIPS(vips_recomb_hip))

static void
vips_recomb_hip_args(VipsRecombHipClass *class)
{
	VIPS_ARG_IMAGE(class, "m", 102, "M", "Matrix of coefficients",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsRecombHip, m));
}

static void
vips_recomb_hip_init(VipsRecombHip *recomb)
{
}

/* relational_const_hip / boolean_const_hip / bandjoin_const_hip / extract_band_hip / bandmean_hip / bandbool_hip:
 * arithmetic/relational.c:560-585, boolean.c:553-576, conversion/bandjoin.c:395-421, extract.c:419-456,
 * bandmean.c:173-192, bandbool.c:218-246.  Pel by pel: an image over the HBM budget goes through in row strips of the
 * same rows, each strip one call of the region form straight into the strip's output.  The output's header is the
 * original's (a one-band image against n constants makes n bands).  Complex images, and more constants than the kernels
 * keep, are the original's (hip_wants_original). */
typedef struct _VipsLogicConstHip {
	VipsHipOp parent_instance;
	int operation; /* VipsOperationRelational / VipsOperationBoolean */
	VipsArrayDouble *c;
	int band, n;
} VipsLogicConstHip;

typedef VipsLogicConstHip VipsRelationalConstHip;
typedef VipsLogicConstHip VipsBooleanConstHip;
typedef VipsLogicConstHip VipsBandjoinConstHip;
typedef VipsLogicConstHip VipsExtractBandHip;
typedef VipsLogicConstHip VipsBandmeanHip;
typedef VipsLogicConstHip VipsBandboolHip;

static const double *
logic_hip_constants(VipsHipOp *op, int *n)
{
	VipsLogicConstHip *logic = (VipsLogicConstHip *) op;

	*n = 0;
	return logic->c ? vips_array_double_get(logic->c, n) : NULL;
}

static int
vips_relational_const_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	int n;
	const double *c = logic_hip_constants(op, &n);

	return vips_hip_relational_const(in, out, ((VipsLogicConstHip *) op)->operation, c, n);
}

static int
vips_boolean_const_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	int n;
	const double *c = logic_hip_constants(op, &n);

	return vips_hip_boolean_const(in, out, ((VipsLogicConstHip *) op)->operation, c, n);
}

static int
vips_bandjoin_const_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	int n;
	const double *c = logic_hip_constants(op, &n);

	return vips_hip_bandjoin_const(in, out, c, n);
}

static int
vips_extract_band_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsLogicConstHip *logic = (VipsLogicConstHip *) op;

	return vips_hip_extract_band(in, out, logic->band, logic->n);
}

static int
vips_bandmean_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_hip_bandmean(in, out);
}

static int
vips_bandbool_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	return vips_hip_bandbool(in, out, ((VipsLogicConstHip *) op)->operation);
}

/* (no plan: the region forms take the operation's own arguments) */
static int
vips_relational_const_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	int n;
	const double *c = logic_hip_constants(op, &n);

	return vips_hip_relational_const_gen(((VipsLogicConstHip *) op)->operation, c, n, in, out);
}

static int
vips_boolean_const_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	int n;
	const double *c = logic_hip_constants(op, &n);

	return vips_hip_boolean_const_gen(((VipsLogicConstHip *) op)->operation, c, n, in, out);
}

static int
vips_bandjoin_const_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	int n;
	const double *c = logic_hip_constants(op, &n);

	return vips_hip_bandjoin_const_gen(c, n, in, out);
}

static int
vips_extract_band_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_extract_band_gen(((VipsLogicConstHip *) op)->band, in, out);
}

static int
vips_bandmean_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_bandmean_gen(in, out);
}

static int
vips_bandbool_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	return vips_hip_bandbool_gen(((VipsLogicConstHip *) op)->operation, in, out);
}

#define LOGIC_HIP_STRIPS(type_name) \
	class->strip_open = vips_invert_hip_strip_open; \
	class->strip_need = vips_linear_hip_strip_need; \
	class->strip_run = type_name##_strip_run; \
	class->strip_close = vips_invert_hip_strip_close;

HIP_SUBCLASS_FULL(VipsRelationalConstHip, vips_relational_const_hip, "relational_const_hip",
	"relational operations against a constant (MI355X)", LOGIC_HIP_STRIPS(vips_relational_const_hip))
HIP_SUBCLASS_FULL(VipsBooleanConstHip, vips_boolean_const_hip, "boolean_const_hip",
	"boolean operations against a constant (MI355X)", LOGIC_HIP_STRIPS(vips_boolean_const_hip))
HIP_SUBCLASS_FULL(VipsBandjoinConstHip, vips_bandjoin_const_hip, "bandjoin_const_hip",
	"append a constant band to an image (MI355X)", LOGIC_HIP_STRIPS(vips_bandjoin_const_hip))
HIP_SUBCLASS_FULL(VipsExtractBandHip, vips_extract_band_hip, "extract_band_hip", "extract band from an image (MI355X)",
	LOGIC_HIP_STRIPS(vips_extract_band_hip))
HIP_SUBCLASS_FULL(VipsBandmeanHip, vips_bandmean_hip, "bandmean_hip", "band-wise average (MI355X)",
	LOGIC_HIP_STRIPS(vips_bandmean_hip))
HIP_SUBCLASS_FULL(VipsBandboolHip, vips_bandbool_hip, "bandbool_hip", "boolean operation across image bands (MI355X)",
	LOGIC_HIP_STRIPS(vips_bandbool_hip))

static void
vips_relational_const_hip_args(VipsRelationalConstHipClass *class)
{
	VIPS_ARG_ENUM(class, "relational", 200, "Operation", "Relational to perform",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsLogicConstHip, operation),
		VIPS_TYPE_OPERATION_RELATIONAL, VIPS_OPERATION_RELATIONAL_EQUAL);
	VIPS_ARG_BOXED(class, "c", 201, "c", "Array of constants",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsLogicConstHip, c), VIPS_TYPE_ARRAY_DOUBLE);
}

static void
vips_boolean_const_hip_args(VipsBooleanConstHipClass *class)
{
	VIPS_ARG_ENUM(class, "boolean", 200, "Operation", "Boolean to perform",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsLogicConstHip, operation),
		VIPS_TYPE_OPERATION_BOOLEAN, VIPS_OPERATION_BOOLEAN_AND);
	VIPS_ARG_BOXED(class, "c", 201, "c", "Array of constants",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsLogicConstHip, c), VIPS_TYPE_ARRAY_DOUBLE);
}

static void
vips_bandjoin_const_hip_args(VipsBandjoinConstHipClass *class)
{
	VIPS_ARG_BOXED(class, "c", 12, "Constants", "Array of constants to add",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsLogicConstHip, c), VIPS_TYPE_ARRAY_DOUBLE);
}

static void
vips_extract_band_hip_args(VipsExtractBandHipClass *class)
{
	VIPS_ARG_INT(class, "band", 3, "Band", "Band to extract",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsLogicConstHip, band), 0, VIPS_MAX_COORD, 0);
	VIPS_ARG_INT(class, "n", 4, "n", "Number of bands to extract",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsLogicConstHip, n), 1, VIPS_MAX_COORD, 1);
}

static void
vips_bandmean_hip_args(VipsBandmeanHipClass *class)
{
}

static void
vips_bandbool_hip_args(VipsBandboolHipClass *class)
{
	VIPS_ARG_ENUM(class, "boolean", 200, "Operation", "Boolean to perform",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsLogicConstHip, operation),
		VIPS_TYPE_OPERATION_BOOLEAN, VIPS_OPERATION_BOOLEAN_AND);
}

static void
vips_relational_const_hip_init(VipsRelationalConstHip *logic)
{
}

static void
vips_boolean_const_hip_init(VipsBooleanConstHip *logic)
{
}

static void
vips_bandjoin_const_hip_init(VipsBandjoinConstHip *logic)
{
}

static void
vips_extract_band_hip_init(VipsExtractBandHip *logic)
{
	logic->n = 1;
}

static void
vips_bandmean_hip_init(VipsBandmeanHip *logic)
{
}

static void
vips_bandbool_hip_init(VipsBandboolHip *logic)
{
}

/* replicate_hip, wrap_hip, grid_hip (conversion/replicate.c, wrap.c, grid.c) and zoom_hip, subsample_hip (zoom.c,
 * subsample.c).  The header is the original's (hip_twin_header: wrap's Xoffset / Yoffset come with it, and its build
 * has said "bad grid geometry", "zoom factors too large" or "image has shrunk to nothing" by then).  The region forms
 * work in whole-image coordinates; a strip reads the rows vips_hip_replicate_need / vips_hip_grid_need name, which is
 * every row once a strip crosses a period or a grid has more than one tile across.  wrap_hip is vips_hip_replicate_gen
 * with the offset.  (arrayjoin takes an array of images and these classes take one: it has no class here.) */
typedef struct _VipsCellsHip {
	VipsHipOp parent_instance;
	int across, down, tile_height;
	int x, y;
	int xfac, yfac;
	gboolean point;
} VipsCellsHip;

typedef VipsCellsHip VipsReplicateHip;
typedef VipsCellsHip VipsWrapHip;
typedef VipsCellsHip VipsGridHip;
typedef VipsCellsHip VipsZoomHip;
typedef VipsCellsHip VipsSubsampleHip;

static int
vips_cells_hip_strip_open(VipsHipOp *op, VipsImage *in, void **plan)
{
	/* the arguments are the plan */
	*plan = op;

	return 0;
}

static void
vips_cells_hip_strip_close(VipsHipOp *op, void *plan)
{
}

static int
vips_replicate_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsCellsHip *cells = (VipsCellsHip *) op;

	return vips_hip_replicate(in, out, cells->across, cells->down);
}

/* Where the output's pel (0, 0) lies in its period: for wrap_hip what the original's build put into the header
 * (wrap.c:99-100), for replicate_hip the corner. */
static void
cells_hip_origin(VipsHipOp *op, int *x0, int *y0)
{
	const gboolean wrap = strcmp(VIPS_OBJECT_GET_CLASS(op)->nickname, "wrap_hip") == 0;

	*x0 = wrap ? op->out->Xoffset : 0;
	*y0 = wrap ? op->out->Yoffset : 0;
}

static void
vips_replicate_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	int x0, y0, need[4];

	cells_hip_origin(op, &x0, &y0);
	vips_hip_replicate_need(op->ready->Xsize, op->ready->Ysize, x0, y0, 0, out_top, op->out->Xsize, out_rows, need);
	*in_top = need[1];
	*in_rows = need[3];
}

static int
vips_replicate_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	int x0, y0;

	cells_hip_origin(op, &x0, &y0);

	return vips_hip_replicate_gen(x0, y0, in, out);
}

static int
vips_wrap_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsCellsHip *cells = (VipsCellsHip *) op;

	return vips_hip_wrap(in, out, cells->x, cells->y, vips_object_argument_isset(VIPS_OBJECT(op), "x"),
		vips_object_argument_isset(VIPS_OBJECT(op), "y"));
}

static int
vips_grid_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsCellsHip *cells = (VipsCellsHip *) op;

	return vips_hip_grid(in, out, cells->tile_height, cells->across, cells->down);
}

static void
vips_grid_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	VipsCellsHip *cells = (VipsCellsHip *) op;
	int need[4];

	vips_hip_grid_need(op->ready->Xsize, op->ready->Ysize, cells->tile_height, cells->across, 0, out_top, op->out->Xsize,
		out_rows, need);
	*in_top = need[1];
	*in_rows = need[3];
}

static int
vips_grid_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	VipsCellsHip *cells = (VipsCellsHip *) op;

	return vips_hip_grid_gen(cells->tile_height, cells->across, in, out);
}

static int
vips_zoom_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsCellsHip *cells = (VipsCellsHip *) op;

	return vips_hip_zoom(in, out, cells->xfac, cells->yfac);
}

static void
vips_zoom_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	VipsCellsHip *cells = (VipsCellsHip *) op;

	*in_top = out_top / cells->yfac;
	*in_rows = (out_top + out_rows - 1) / cells->yfac - *in_top + 1;
}

static int
vips_zoom_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	VipsCellsHip *cells = (VipsCellsHip *) op;

	return vips_hip_zoom_gen(in, out, cells->xfac, cells->yfac);
}

static int
vips_subsample_hip_compute(VipsHipOp *op, VipsHipImage *in, VipsHipImage **out)
{
	VipsCellsHip *cells = (VipsCellsHip *) op;

	return vips_hip_subsample(in, out, cells->xfac, cells->yfac);
}

static void
vips_subsample_hip_strip_need(VipsHipOp *op, void *plan, int out_top, int out_rows, int *in_top, int *in_rows)
{
	VipsCellsHip *cells = (VipsCellsHip *) op;

	*in_top = out_top * cells->yfac;
	*in_rows = (out_rows - 1) * cells->yfac + 1;
}

static int
vips_subsample_hip_strip_run(VipsHipOp *op, void *plan, const VipsHipRegion *in, const VipsHipRegion *out)
{
	VipsCellsHip *cells = (VipsCellsHip *) op;

	return vips_hip_subsample_gen(in, out, cells->xfac, cells->yfac);
}

#define vips_replicate_hip_strip_open vips_cells_hip_strip_open
#define vips_replicate_hip_strip_close vips_cells_hip_strip_close
#define vips_wrap_hip_strip_open vips_cells_hip_strip_open
#define vips_wrap_hip_strip_need vips_replicate_hip_strip_need
#define vips_wrap_hip_strip_run vips_replicate_hip_strip_run
#define vips_wrap_hip_strip_close vips_cells_hip_strip_close
#define vips_grid_hip_strip_open vips_cells_hip_strip_open
#define vips_grid_hip_strip_close vips_cells_hip_strip_close
#define vips_zoom_hip_strip_open vips_cells_hip_strip_open
#define vips_zoom_hip_strip_close vips_cells_hip_strip_close
#define vips_subsample_hip_strip_open vips_cells_hip_strip_open
#define vips_subsample_hip_strip_close vips_cells_hip_strip_close

HIP_SUBCLASS_FULL(VipsReplicateHip, vips_replicate_hip, "replicate_hip", "replicate an image (MI355X)", HIP_STRIPS(vips_replicate_hip))
HIP_SUBCLASS_FULL(VipsWrapHip, vips_wrap_hip, "wrap_hip", "wrap image origin (MI355X)", HIP_STRIPS(vips_wrap_hip))
HIP_SUBCLASS_FULL(VipsGridHip, vips_grid_hip, "grid_hip", "grid an image (MI355X)", HIP_STRIPS(vips_grid_hip))
HIP_SUBCLASS_FULL(VipsZoomHip, vips_zoom_hip, "zoom_hip", "zoom an image (MI355X)", HIP_STRIPS(vips_zoom_hip))
HIP_SUBCLASS_FULL(VipsSubsampleHip, vips_subsample_hip, "subsample_hip", "subsample an image (MI355X)", HIP_STRIPS(vips_subsample_hip))

static void
vips_replicate_hip_args(VipsReplicateHipClass *class)
{
	VIPS_ARG_INT(class, "across", 4, "Across", "Repeat this many times horizontally",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsCellsHip, across), 1, 1000000, 1);
	VIPS_ARG_INT(class, "down", 5, "Down", "Repeat this many times vertically",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsCellsHip, down), 1, 1000000, 1);
}

static void
vips_wrap_hip_args(VipsWrapHipClass *class)
{
	VIPS_ARG_INT(class, "x", 3, "x", "Left edge of input in output",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsCellsHip, x), -VIPS_MAX_COORD, VIPS_MAX_COORD, 0);
	VIPS_ARG_INT(class, "y", 4, "y", "Top edge of input in output",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsCellsHip, y), -VIPS_MAX_COORD, VIPS_MAX_COORD, 0);
}

static void
vips_grid_hip_args(VipsGridHipClass *class)
{
	VIPS_ARG_INT(class, "tile_height", 3, "Tile height", "Chop into tiles this high",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsCellsHip, tile_height), 1, 10000000, 128);
	VIPS_ARG_INT(class, "across", 4, "Across", "Number of tiles across",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsCellsHip, across), 1, 10000000, 1);
	VIPS_ARG_INT(class, "down", 5, "Down", "Number of tiles down",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsCellsHip, down), 1, 10000000, 1);
}

static void
cells_hip_factor_args(VipsHipOpClass *class)
{
	VIPS_ARG_INT(class, "xfac", 3, "Xfac", "Horizontal factor",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsCellsHip, xfac), 1, VIPS_MAX_COORD, 1);
	VIPS_ARG_INT(class, "yfac", 4, "Yfac", "Vertical factor",
		VIPS_ARGUMENT_REQUIRED_INPUT, G_STRUCT_OFFSET(VipsCellsHip, yfac), 1, VIPS_MAX_COORD, 1);
}

static void
vips_zoom_hip_args(VipsZoomHipClass *class)
{
	cells_hip_factor_args(class);
}

static void
vips_subsample_hip_args(VipsSubsampleHipClass *class)
{
	cells_hip_factor_args(class);
	VIPS_ARG_BOOL(class, "point", 5, "Point", "Point sample",
		VIPS_ARGUMENT_OPTIONAL_INPUT, G_STRUCT_OFFSET(VipsCellsHip, point), FALSE);
}

static void
vips_cells_hip_init(VipsCellsHip *cells)
{
	cells->across = cells->down = 1;
	cells->tile_height = 128;
	cells->xfac = cells->yfac = 1;
}

static void
vips_replicate_hip_init(VipsReplicateHip *cells)
{
	vips_cells_hip_init(cells);
}

static void
vips_wrap_hip_init(VipsWrapHip *cells)
{
	vips_cells_hip_init(cells);
}

static void
vips_grid_hip_init(VipsGridHip *cells)
{
	vips_cells_hip_init(cells);
}

static void
vips_zoom_hip_init(VipsZoomHip *cells)
{
	vips_cells_hip_init(cells);
}

static void
vips_subsample_hip_init(VipsSubsampleHip *cells)
{
	vips_cells_hip_init(cells);
}
