// vips_sharpen on images in HBM, and the batched thumbnail pipeline (vips_resize then vips_sharpen on n images): the
// host side -- sharpen.c's LUT and its caches, the one-kernel sharpen's conditions, the batch scheduler over CU
// partitions and devices, the C ABI.  The kernels are colour_sharpen.h (in colour.hip) and resize_sharpen.hip.
#include "colour.h"
#include "conv.h"
#include "reduce_u8.h"

#include <atomic>
#include <cmath>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace vh;

namespace {

// the sharpen LUT (sharpen.c:230-257), cached by its parameters
struct LutKey {
	int device;
	double p[5];
	bool operator==(const LutKey &o) const { return device == o.device && memcmp(p, o.p, sizeof(p)) == 0; }
};
typedef std::shared_ptr<int> LutPtr;
// (leaked on purpose, like the convolution caches: no device frees at exit)
std::mutex &g_lut_mutex = *new std::mutex;
std::list<std::pair<LutKey, LutPtr>> &g_lut_cache = *new std::list<std::pair<LutKey, LutPtr>>;

// sharpen.c:230-257
void sharpen_lut_host(double x1, double y2, double y3, double m1, double m2, std::vector<int> &lut)
{
	lut.resize(65536);
	for (int i = 0; i < 65536; i++) {
		double v = (i - 32767) / 327.67;
		double y;

		if (v < -x1)
			y = (v + x1) * m2 + -x1 * m1;
		else if (v < x1)
			y = v * m1;
		else
			y = (v - x1) * m2 + x1 * m1;

		if (y < -y3)
			y = -y3;
		if (y > y2)
			y = y2;

		lut[i] = rint(y * 327.67);
	}
}

LutPtr sharpen_lut_cached(double x1, double y2, double y3, double m1, double m2)
{
	if (ensure_init())
		return LutPtr();
	LutKey key = { current_device(), { x1, y2, y3, m1, m2 } };
	{
		std::lock_guard<std::mutex> lock(g_lut_mutex);
		for (auto it = g_lut_cache.begin(); it != g_lut_cache.end(); ++it)
			if (it->first == key) {
				g_lut_cache.splice(g_lut_cache.begin(), g_lut_cache, it);
				return g_lut_cache.front().second;
			}
	}
	std::vector<int> lut;
	sharpen_lut_host(x1, y2, y3, m1, m2, lut);
	int *d_lut = (int *) upload(lut.data(), lut.size() * sizeof(int));
	if (!d_lut)
		return LutPtr();
	LutPtr l(d_lut, [](int *d) { vips_hip_free(d); });
	std::lock_guard<std::mutex> lock(g_lut_mutex);
	g_lut_cache.emplace_front(key, l);
	while (g_lut_cache.size() > 16)
		g_lut_cache.pop_back();
	return l;
}

// the window of sharpen's LUT that is not constant (sharpen.c:230-257 is flat outside the bends), on the device
// as shorts: what colour_sharpen.h's all-in-LDS sharpen kernel copies into LDS.  A window of n = 0 with lut_win =
// nullptr: this LUT does not fit (the callers take the kernel that reads the LUT through global memory)
std::shared_ptr<vh::SharpenLutWindow> sharpen_lut_window_cached(double x1, double y2, double y3, double m1, double m2)
{
	// (leaked on purpose, like g_lut_cache: the deleter frees device memory, which must not happen from a static
	// destructor after the runtime's own have run)
	static std::mutex &mutex = *new std::mutex;
	static std::list<std::pair<LutKey, std::shared_ptr<vh::SharpenLutWindow>>> &cache =
		*new std::list<std::pair<LutKey, std::shared_ptr<vh::SharpenLutWindow>>>;
	LutKey key = { current_device(), { x1, y2, y3, m1, m2 } };
	std::lock_guard<std::mutex> lock(mutex);
	for (auto it = cache.begin(); it != cache.end(); ++it)
		if (it->first == key) {
			cache.splice(cache.begin(), cache, it);
			return cache.front().second;
		}
	std::vector<int> lut;
	sharpen_lut_host(x1, y2, y3, m1, m2, lut);
	int lo = 0, hi = 65535;
	while (lo < 65536 && lut[lo] == lut[0])
		lo++;
	while (hi >= 0 && lut[hi] == lut[65535])
		hi--;
	std::shared_ptr<vh::SharpenLutWindow> w(new vh::SharpenLutWindow, [](vh::SharpenLutWindow *p) {
		vips_hip_free(const_cast<short *>(p->lut_win));
		delete p;
	});
	w->below = lut[0];
	w->above = lut[65535];
	// the run of zeros around a difference of 0 (m1 = 0, the default: |difference| < x1): the pixels sharpen leaves alone
	w->zero_lo = 1;
	w->zero_hi = 0;
	if (lut[32768] == 0) {
		int zl = 32768, zh = 32768;
		while (zl > 0 && lut[zl - 1] == 0)
			zl--;
		while (zh < 65535 && lut[zh + 1] == 0)
			zh++;
		w->zero_lo = zl - 32768;
		w->zero_hi = zh - 32768;
	}
	w->lo = lo < 65536 ? lo : 0;
	w->n = lo < 65536 && hi >= lo ? hi - lo + 1 : 0;
	w->lut_win = nullptr;
	bool ok = w->n <= 6144;
	std::vector<short> sv((size_t) w->n + 1, 0);
	for (int k = 0; k < w->n && ok; k++) {
		ok = lut[w->lo + k] >= -32768 && lut[w->lo + k] <= 32767;
		sv[k] = (short) lut[w->lo + k];
	}
	if (ok) {
		w->lut_win = (const short *) upload(sv.data(), sv.size() * sizeof(short));
		if (!w->lut_win)
			vips_hip_error_clear();
	}
	cache.emplace_front(key, w);
	while (cache.size() > 16)
		cache.pop_back();
	return w;
}

} // namespace

extern "C" {

// vips_sharpen_build, convolution/sharpen.c:171-302
// vips_sharpen on n 3-band uchar sRGB images of one size (every thumbnail): the LabS round trip,
// the blur of L and the LUT in one kernel (colour_sharpen.h sharpen_fused_u8) when the blur mask has at
// most 5 taps.  0 = done (out[] filled), 1 = not that kernel's case, -1 = error
static int sharpen_fused_images(VipsHipImage *const *in, int n_images, VipsHipImage **out, double sigma, double x1,
	double y2, double y3, double m1, double m2)
{
	for (int i = 0; i < n_images; i++)
		if (!in[i] || in[i]->format != VIPS_HIP_FORMAT_UCHAR || in[i]->bands != 3 ||
			in[i]->interpretation != VIPS_HIP_INTERPRETATION_sRGB ||
			image_guess_interpretation(in[i]) != VIPS_HIP_INTERPRETATION_sRGB || in[i]->width != in[0]->width ||
			in[i]->height != in[0]->height)
			return 1;
	const Route *to = route_find(VIPS_HIP_INTERPRETATION_sRGB, VIPS_HIP_INTERPRETATION_LABS);
	const Route *from = route_find(VIPS_HIP_INTERPRETATION_LABS, VIPS_HIP_INTERPRETATION_sRGB);
	const int n = vips_hip_gaussmat(sigma, 0.1, 1, VIPS_HIP_PRECISION_INTEGER, nullptr, 0, nullptr);
	if (!(to && from && to->n > 0 && from->n > 0 && n >= 1 && n <= 5))
		return 1;
	std::vector<double> mask(n);
	double scale = 1.0;
	if (vips_hip_gaussmat(sigma, 0.1, 1, VIPS_HIP_PRECISION_INTEGER, mask.data(), n, &scale) < 0)
		return -1;
	// the convi C path's integers: rint of the mask and of its scale (convi.c:886-915); zero taps
	// are squeezed out by the reference: same sums
	std::vector<int> coef(n);
	for (int k = 0; k < n; k++)
		coef[k] = (int) rint(mask[k]);
	LutPtr lut = sharpen_lut_cached(x1, y2, y3, m1, m2);
	if (!lut)
		return -1;
	std::vector<ImageRef> o(n_images);
	std::vector<VipsHipRegion> ri(n_images), ro(n_images);
	std::vector<const VipsHipRegion *> pi(n_images), po(n_images);
	for (int i = 0; i < n_images; i++) {
		o[i].im = vips_hip_image_new(in[i]->width, in[i]->height, 3, VIPS_HIP_FORMAT_UCHAR, VIPS_HIP_INTERPRETATION_sRGB);
		if (!o[i].im)
			return -1;
		vips_hip_image_region(in[i], &ri[i]);
		vips_hip_image_region(o[i].im, &ro[i]);
		pi[i] = &ri[i];
		po[i] = &ro[i];
	}
	std::shared_ptr<vh::SharpenLutWindow> win = sharpen_lut_window_cached(x1, y2, y3, m1, m2);
	const int r = vh::sharpen_fused_u8(pi.data(), po.data(), n_images, to->steps, to->n, from->steps, from->n,
		coef.data(), n, (int) rint(scale), lut.get(), win.get());
	if (r)
		return r;
	for (int i = 0; i < n_images; i++)
		out[i] = o[i].release();
	return 0;
}

int vips_hip_sharpen(VipsHipImage *in, VipsHipImage **out, double sigma, double x1, double y2,
	double y3, double m1, double m2)
{
	if (in && vh::bind_to(in)) // run where the pixels live
		return -1;
	if (!in || !out) {
		error("sharpen", "null argument");
		return -1;
	}
	const int old_interpretation = in->interpretation;
	{
		const int r = sharpen_fused_images(&in, 1, out, sigma, x1, y2, y3, m1, m2);
		if (r <= 0)
			return r;
	}
	ImageRef labs;
	if (vips_hip_colourspace(in, &labs.im, VIPS_HIP_INTERPRETATION_LABS))
		return -1;
	if (labs.im->bands < 3) {
		error("sharpen", "image must have at least 3 bands");
		return -1;
	}

	// "Stop at 10% of max ... We always sharpen a short, so there's no point using a
	// float mask."
	int width = vips_hip_gaussmat(sigma, 0.1, 1, VIPS_HIP_PRECISION_INTEGER, nullptr, 0, nullptr);
	if (width < 0)
		return -1;
	std::vector<double> mask(width);
	double scale = 1.0;
	if (vips_hip_gaussmat(sigma, 0.1, 1, VIPS_HIP_PRECISION_INTEGER, mask.data(), width, &scale) < 0)
		return -1;

	// vips_cast_short: colourspace(LABS) already produced short
	ImageRef shorts;
	VipsHipImage *cur = labs.im;
	if (cur->format != VIPS_HIP_FORMAT_SHORT) {
		if (cast_image(cur, &shorts.im, VIPS_HIP_FORMAT_SHORT))
			return -1;
		cur = shorts.im;
	}

	LutPtr lut = sharpen_lut_cached(x1, y2, y3, m1, m2);
	if (!lut)
		return -1;
	int *d_lut = lut.get();

	// extract L, blur it with the integer separable mask (sharpen.c:274-278)
	ImageRef L(vips_hip_image_new(cur->width, cur->height, 1, VIPS_HIP_FORMAT_SHORT,
		cur->interpretation));
	ImageRef blurred, sharp(vips_hip_image_new(cur->width, cur->height, cur->bands,
							   VIPS_HIP_FORMAT_SHORT, VIPS_HIP_INTERPRETATION_LABS));
	int result = -1;
	if (L.im && sharp.im) {
		VipsHipRegion rc, rl;
		vips_hip_image_region(cur, &rc);
		vips_hip_image_region(L.im, &rl);
		if (!band_cast(&rc, 0, &rl, 0, 1) &&
			!vips_hip_convsep(L.im, &blurred.im, mask.data(), width, scale, 0.0,
				VIPS_HIP_PRECISION_INTEGER)) {
			VipsHipRegion rb, rs;
			vips_hip_image_region(blurred.im, &rb);
			vips_hip_image_region(sharp.im, &rs);
			result = vips_hip_sharpen_gen(d_lut, &rc, &rb, &rs);
		}
	}
	if (result)
		return -1;

	// back to where we came from (sharpen.c:295-297)
	return vips_hip_colourspace(sharp.im, out, old_interpretation);
}

// vips_sharpen's blur mask as the convi C path's integers (sharpen.c:214-218, convi.c:886-915) when
// it has at most 5 taps -- the case of the fused sharpen kernels; false: a wider mask (or an error,
// which the unfused path then reports)
static bool sharpen_small_mask(double sigma, std::vector<int> &coef, int *scale)
{
	const int n = vips_hip_gaussmat(sigma, 0.1, 1, VIPS_HIP_PRECISION_INTEGER, nullptr, 0, nullptr);
	if (n < 1 || n > 5)
		return false;
	std::vector<double> mask(n);
	double s = 1.0;
	if (vips_hip_gaussmat(sigma, 0.1, 1, VIPS_HIP_PRECISION_INTEGER, mask.data(), n, &s) < 0) {
		vips_hip_error_clear();
		return false;
	}
	coef.resize(n);
	for (int k = 0; k < n; k++)
		coef[k] = (int) rint(mask[k]);
	*scale = (int) rint(s);
	return true;
}

static bool sharpen_images_fusable(VipsHipImage *const *in, int n)
{
	for (int i = 0; i < n; i++)
		if (!in[i] || in[i]->format != VIPS_HIP_FORMAT_UCHAR || in[i]->bands != 3 ||
			in[i]->interpretation != VIPS_HIP_INTERPRETATION_sRGB || in[i]->width != in[0]->width ||
			in[i]->height != in[0]->height)
			return false;
	return n > 0;
}

// The two CU partitions of the batched pipeline (see vips_hip_resize_sharpen_batch): streams
// restricted to 3/4 and 1/4 of the CUs: the low and the high run of consecutive mask bits.  (What
// the runtime honours on this part, measured by tools/c4_masks.py: runs of at least 8 consecutive
// bits restrict a queue, in effect in groups of 32 CUs -- 48 or 56 bits behave like 32; masks
// interleaved finer than that leave it on every CU.)  Made once per device and kept (a masked
// stream is a hardware queue with a fixed mask).
struct BatchStreams {
	hipStream_t resize = nullptr, sharpen = nullptr;
};
static BatchStreams *batch_streams()
{
	static std::mutex mutex;
	static std::map<int, BatchStreams> by_device;
	int device = 0;
	if (hipGetDevice(&device) != hipSuccess)
		return nullptr;
	std::lock_guard<std::mutex> lock(mutex);
	auto it = by_device.find(device);
	if (it != by_device.end())
		return it->second.resize ? &it->second : nullptr;
	BatchStreams &bs = by_device[device];
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) != hipSuccess)
		return nullptr;
	const int cus = prop.multiProcessorCount;
	const int share = getenv("VIPS_HIP_BATCH_SHARPEN_CUS") ? atoi(getenv("VIPS_HIP_BATCH_SHARPEN_CUS")) : cus / 4;
	if (share == 0) {
		// $VIPS_HIP_BATCH_SHARPEN_CUS=0: two plain streams, both kernels on every CU (the sharpen's at the lowest
		// priority the device offers: it fills what the resize leaves)
		int least = 0, greatest = 0;
		(void) hipDeviceGetStreamPriorityRange(&least, &greatest);
		if (hipStreamCreateWithPriority(&bs.resize, hipStreamNonBlocking, greatest) != hipSuccess ||
			hipStreamCreateWithPriority(&bs.sharpen, hipStreamNonBlocking, least) != hipSuccess) {
			if (bs.resize) // the second failed
				(void) hipStreamDestroy(bs.resize);
			bs.resize = bs.sharpen = nullptr;
			(void) hipGetLastError();
			return nullptr;
		}
		return &bs;
	}
	if (cus < 16 || cus > 1024 || share < 8 || share > cus - 8)
		return nullptr;
	std::vector<uint32_t> lo((cus + 31) / 32, 0u), hi((cus + 31) / 32, 0u);
	for (int i = 0; i < cus; i++)
		(i < cus - share ? lo : hi)[i / 32] |= 1u << (i % 32);
	if (hipExtStreamCreateWithCUMask(&bs.resize, (uint32_t) lo.size(), lo.data()) != hipSuccess ||
		hipExtStreamCreateWithCUMask(&bs.sharpen, (uint32_t) hi.size(), hi.data()) != hipSuccess) {
		if (bs.resize) // the second failed
			(void) hipStreamDestroy(bs.resize);
		bs.resize = bs.sharpen = nullptr; // (the plain one-stream order then)
		(void) hipGetLastError();
		return nullptr;
	}
	return &bs;
}
// BASELINE config 4, the batched thumbnail pipeline: vips_resize(scale) [then vips_sharpen()] on
// n independent images.  libvips runs such a batch as n pipelines over its thread pool
// (iofuncs/threadpool.c:625); here n_threads host threads each take the next image, every thread
// on its own stream: the many small kernels of one image's sharpen stage overlap the two big
// streaming kernels of the next images' resize instead of each paying its launch latency alone.
// sigma < 0 skips the sharpen.  Returns the number of images that failed (their outs[] are
// NULL; the first error message is left in the caller's error buffer); all work is complete
// on return.
// ... on the device the calling thread drives (every image of `in` lives there)
// wait = false: a uniform batch returns as soon as it is queued (everything it queued is ordered on
// the calling thread's stream: the join below); any other batch, and every failure, waits as before
static int resize_sharpen_batch_here(VipsHipImage *const *in, int n, VipsHipImage **out, double scale, int kernel,
	double gap, double sigma, double x1, double y2, double y3, double m1, double m2, int n_threads, bool wait = true)
{
	if (n_threads < 1)
		n_threads = 1;
	if (n_threads > n)
		n_threads = n;
	for (int i = 0; i < n; i++)
		out[i] = nullptr;
	// A batch of uchar images of one size whose resize is the streaming kernel's case: one launch
	// per 64 images for the whole resize chain (resize_stream.hip) and one for the sharpen.
	//
	// The resize chain is bound by HBM, the sharpen by the FP64 pipe.  Queued one behind the other
	// on one stream they cost the sum of their times (0.040 + 0.010 ms per 8192 x 8192 image);
	// left to share every CU (two plain streams) each gets in the other's way and the sum stays
	// (round 2: 0.044 + 0.016 side by side).  So the CUs are PARTITIONED: the resize of chunk k + 1
	// runs on a stream masked to 3/4 of the CUs of every XCD (hipExtStreamCreateWithCUMask) next to
	// the sharpen of chunk k on the other quarter -- measured on the MI355X (tools/c4_cumask.py):
	// resize 0.0405 ms per image on 256 CUs, 0.0440 on 192; sharpen x 4 on 64 CUs = about the same
	// time, so a pair of chunks takes what the resize alone takes on 192 CUs.  The first chunk's
	// resize and the last chunk's sharpen have nothing to run beside and take every CU.  $VIPS_HIP_BATCH_OVERLAP=0: one
	// stream, one stage after the other.
	if (n > 0 && !getenv("VIPS_HIP_NO_BATCH_LAUNCH")) {
		const int chunk = 64;
		// resize and sharpen of 3-band sRGB images in ONE kernel (resize_sharpen.hip): nothing to
		// partition, no thumbnail in memory between the two.  Bit-exact, but on the MI355X the
		// sharpen's arithmetic inside the streaming blocks costs more than the partition it removes
		// (0.051 ms per 8192 x 8192 image against 0.043: DESIGN.md 3.2), so it runs on request only:
		// $VIPS_HIP_RESIZE_SHARPEN=1
		std::vector<int> coef;
		int mask_scale = 1;
		const bool small_mask = sigma >= 0.0 && sharpen_small_mask(sigma, coef, &mask_scale);
		const bool fusable = small_mask && sharpen_images_fusable(in, n);
		const char *one_kernel = getenv("VIPS_HIP_RESIZE_SHARPEN");
		if (fusable && one_kernel && atoi(one_kernel) > 0) {
			std::vector<int> lut;
			sharpen_lut_host(x1, y2, y3, m1, m2, lut);
			const int r = vh::resize_sharpen_batch_u8(in, n, out, scale, kernel, gap, coef.data(), (int) coef.size(),
				mask_scale, lut.data());
			if (r < 0)
				return -1;
			if (r == 0) {
				if (wait && vips_hip_synchronize()) {
					for (int i = 0; i < n; i++) {
						vips_hip_image_unref(out[i]);
						out[i] = nullptr;
					}
					return -1;
				}
				return 0;
			}
		}
		std::vector<ImageRef> small(n); // held to the end: several streams read and write them
		std::vector<VipsHipImage *> ps(n, nullptr);
		const int first = n < chunk ? n : chunk;
		const char *ov = getenv("VIPS_HIP_BATCH_OVERLAP");
		// (the partitions only when the ONE-kernel sharpen will run on them: the unfused sharpen takes
		// its temporaries from the pool, which orders reuse within one stream only)
		BatchStreams *bs = sigma >= 0.0 && n > chunk && fusable && !getenv("VIPS_HIP_NO_FUSED_SHARPEN") &&
				!(ov && atoi(ov) == 0)
			? batch_streams()
			: nullptr;
		hipStream_t main_stream = stream();
		std::vector<hipEvent_t> events;
		auto event_on = [&](hipStream_t s) -> hipEvent_t {
			hipEvent_t ev = nullptr;
			if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
				return nullptr;
			events.push_back(ev);
			return hipEventRecord(ev, s) == hipSuccess ? ev : nullptr;
		};
		int bad = 0;
		if (bs) {
			// both partitions start behind whatever the caller queued on its stream
			hipEvent_t ev = event_on(main_stream);
			if (!ev || hipStreamWaitEvent(bs->resize, ev, 0) != hipSuccess || hipStreamWaitEvent(bs->sharpen, ev, 0) != hipSuccess)
				bad = 1;
		}
		// the first chunk's resize has no sharpen to run beside: it takes every CU (the caller's
		// stream), and the resize partition starts behind it
		int r = 0;
		hipEvent_t first_done = nullptr;
		if (!bad) {
			r = vh::resize_batch_u8(in, first, ps.data(), scale, kernel, gap);
			if (bs && r == 0) {
				first_done = event_on(main_stream);
				if (!first_done || hipStreamWaitEvent(bs->resize, first_done, 0) != hipSuccess)
					bad = 1;
			}
		}
		if (r < 0 || bad) {
			for (hipEvent_t ev : events)
				(void) hipEventDestroy(ev);
			return -1;
		}
		if (r == 0) {
			for (int base = 0; base < n && !bad; base += chunk) {
				const int cnt = n - base < chunk ? n - base : chunk;
				const bool last = base + cnt >= n;
				if (base > 0) {
					ScopedStream on(bs ? bs->resize : nullptr);
					const int rr = vh::resize_batch_u8(in + base, cnt, ps.data() + base, scale, kernel, gap);
					if (rr < 0)
						bad = 1;
					else if (rr > 0) // a chunk of another geometry: image by image
						for (int i = base; i < base + cnt && !bad; i++)
							if (!in[i] || vips_hip_resize(in[i], &ps[i], scale, -1.0, kernel, gap))
								bad = 1;
				}
				for (int i = base; i < base + cnt; i++)
					small[i].im = ps[i];
				if (bad)
					break;
				if (sigma < 0.0) {
					for (int i = base; i < base + cnt; i++)
						out[i] = small[i].release();
					continue;
				}
				// the sharpen of this chunk: behind its resize, on the sharpen partition -- the
				// last chunk's on the caller's stream (every CU), which then also waits for the rest
				hipStream_t sharpen_on = nullptr;
				if (bs) {
					sharpen_on = last ? main_stream : bs->sharpen;
					hipEvent_t ev = base == 0 ? first_done : event_on(bs->resize);
					if (!ev || hipStreamWaitEvent(sharpen_on, ev, 0) != hipSuccess)
						bad = 1;
				}
				if (bad)
					break;
				{
					ScopedStream on(sharpen_on);
					int done = sharpen_fused_images(ps.data() + base, cnt, out + base, sigma, x1, y2, y3, m1, m2);
					if (done > 0) {
						// not the one-kernel sharpen's case after all: the separate operations take pool
						// blocks for their temporaries, which are only ordered within ONE stream -- so
						// nothing else of the batch may be in flight around them
						if (bs && (hipStreamSynchronize(bs->resize) != hipSuccess || hipStreamSynchronize(bs->sharpen) != hipSuccess ||
									  hipStreamSynchronize(main_stream) != hipSuccess))
							bad = 1;
						done = 0;
						for (int i = base; i < base + cnt && !done && !bad; i++)
							done = vips_hip_sharpen(ps[i], &out[i], sigma, x1, y2, y3, m1, m2);
						if (bs && hipStreamSynchronize(sharpen_on ? sharpen_on : main_stream) != hipSuccess)
							bad = 1;
					}
					if (done)
						bad = 1;
				}
			}
			if (bs) {
				// the caller's stream ends behind both partitions, so that everything the batch
				// queued is ordered on it
				for (hipStream_t s : { bs->resize, bs->sharpen }) {
					hipEvent_t ev = event_on(s);
					if (!ev || hipStreamWaitEvent(main_stream, ev, 0) != hipSuccess)
						bad = 1;
				}
			}
			// (queued form: the intermediate thumbnails go back to the pool below while the device
			// still reads them -- the pool hands a block to this thread's later work only, and that
			// work is queued behind the join; an event destroyed before it completes is released
			// when it does)
			if (wait || bad) {
				if (vips_hip_synchronize())
					bad = 1;
				if (bs && (hipStreamSynchronize(bs->resize) != hipSuccess || hipStreamSynchronize(bs->sharpen) != hipSuccess))
					bad = 1;
			}
			for (hipEvent_t ev : events)
				(void) hipEventDestroy(ev);
			if (bad) {
				for (int i = 0; i < n; i++) {
					vips_hip_image_unref(out[i]);
					out[i] = nullptr;
				}
				return -1;
			}
			return 0;
		}
		for (hipEvent_t ev : events)
			(void) hipEventDestroy(ev);
	}
	std::atomic<int> next(0), failed(0);
	std::mutex err_mutex;
	std::string first_error;
	auto worker = [&]() {
		for (;;) {
			const int i = next.fetch_add(1);
			if (i >= n)
				break;
			out[i] = nullptr;
			ImageRef small;
			int r = in[i] ? vips_hip_resize(in[i], &small.im, scale, -1.0, kernel, gap) : -1;
			if (!r) {
				if (sigma >= 0.0)
					r = vips_hip_sharpen(small.im, &out[i], sigma, x1, y2, y3, m1, m2);
				else
					out[i] = small.release();
			}
			if (r) {
				out[i] = nullptr;
				failed.fetch_add(1);
				std::lock_guard<std::mutex> lock(err_mutex);
				if (first_error.empty())
					first_error = in[i] ? vips_hip_error_buffer() : "resize_sharpen_batch: null image\n";
				vips_hip_error_clear(); // the error buffer is per thread
			}
		}
	};
	if (n_threads <= 1) {
		worker();
		if (vips_hip_synchronize())
			return -1;
	}
	else {
		std::vector<std::thread> pool;
		// results cross to the caller's thread: every pool thread finishes its stream (and gives
		// it back) before it ends
		for (int t = 0; t < n_threads; t++)
			pool.emplace_back([&]() {
				worker();
				release_thread_stream();
			});
		for (std::thread &t : pool)
			t.join();
	}
	if (!first_error.empty())
		error("resize_sharpen_batch", "%s", first_error.c_str());
	return failed.load();
}

// The batch SCATTER of BASELINE config 4 inside one process: the images of a batch may live on
// several devices (whoever loaded them dealt them out: vips_hip_devices()); each device's share
// runs on a host thread bound to that device -- its own pool, plan caches and streams -- with no
// data moving between devices.  One device: the calling thread does the work itself.
static int resize_sharpen_batch_any(VipsHipImage *const *in, int n, VipsHipImage **out, double scale, int kernel,
	double gap, double sigma, double x1, double y2, double y3, double m1, double m2, int n_threads, bool wait)
{
	if (!in || !out || n < 0) {
		error("resize_sharpen_batch", "null argument");
		return -1;
	}
	if (ensure_init())
		return -1;
	std::map<int, std::vector<int>> by_device;
	for (int i = 0; i < n; i++)
		by_device[in[i] ? in[i]->device : current_device()].push_back(i);
	if (by_device.size() <= 1) {
		if (n > 0 && vh::bind_to(in[by_device.begin()->second[0]]))
			return -1;
		return resize_sharpen_batch_here(in, n, out, scale, kernel, gap, sigma, x1, y2, y3, m1, m2, n_threads, wait);
	}
	for (int i = 0; i < n; i++)
		out[i] = nullptr;
	std::mutex err_mutex;
	std::string first_error;
	std::atomic<int> failed(0);
	std::vector<std::thread> workers;
	for (auto &group : by_device) {
		const int device = group.first;
		const std::vector<int> &idx = group.second;
		workers.emplace_back([&, device]() {
			std::vector<VipsHipImage *> sub_in(idx.size()), sub_out(idx.size(), nullptr);
			for (size_t k = 0; k < idx.size(); k++)
				sub_in[k] = in[idx[k]];
			int r = vips_hip_init(device);
			if (!r)
				r = resize_sharpen_batch_here(sub_in.data(), (int) idx.size(), sub_out.data(), scale, kernel, gap, sigma,
					x1, y2, y3, m1, m2, n_threads);
			for (size_t k = 0; k < idx.size(); k++)
				out[idx[k]] = sub_out[k];
			if (r) {
				failed.fetch_add(r < 0 ? (int) idx.size() : r);
				std::lock_guard<std::mutex> lock(err_mutex);
				if (first_error.empty())
					first_error = vips_hip_error_buffer();
			}
			release_thread_stream(); // results cross to the caller's thread
		});
	}
	for (std::thread &t : workers)
		t.join();
	if (!first_error.empty())
		error("resize_sharpen_batch", "%s", first_error.c_str());
	return failed.load() == n ? -1 : failed.load();
}

int vips_hip_resize_sharpen_batch(VipsHipImage *const *in, int n, VipsHipImage **out, double scale, int kernel,
	double gap, double sigma, double x1, double y2, double y3, double m1, double m2, int n_threads)
{
	return resize_sharpen_batch_any(in, n, out, scale, kernel, gap, sigma, x1, y2, y3, m1, m2, n_threads, true);
}

// ... returning as soon as the batch is QUEUED when it is one the library runs in batch launches on
// the caller's device (the usual case of a thumbnail service: same-sized uchar images): the results
// are then ordered on the calling thread's stream like any other operation's -- use them in stream
// order, or vips_hip_synchronize() -- and the host prepares the next batch while this one runs.
int vips_hip_resize_sharpen_batch_queue(VipsHipImage *const *in, int n, VipsHipImage **out, double scale, int kernel,
	double gap, double sigma, double x1, double y2, double y3, double m1, double m2, int n_threads)
{
	return resize_sharpen_batch_any(in, n, out, scale, kernel, gap, sigma, x1, y2, y3, m1, m2, n_threads, false);
}

} // extern "C"
