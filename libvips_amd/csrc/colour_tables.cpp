// The tables of the colour path, made on the host by the libm calls the reference makes them with (LabQ2sRGB.c:130-160,
// XYZ2Lab.c:92-106) and uploaded once per device: the sRGB tables and the cube-root table, and the LDS-sized forms of
// the cube-root table (cbrt_exact.h, cbrt_quad.h).  Host code only (the cbrt_*.h schemes are __host__ __device__: every
// file here is compiled as HIP).
#include "colour_device.h"
#define VH_CBRT_FN static __host__ __device__ __forceinline__
#include "cbrt_exact.h"
#include "cbrt_quad.h"

#include <cstdlib>
#include <cstring>
#include <cmath>
#include <mutex>

namespace vh {

static std::mutex &g_tables_mutex = *new std::mutex;
// one set per device (the tables are device memory)
static ColourTables g_tables_by_device[64];
#define g_tables (g_tables_by_device[current_device() < 0 ? 0 : current_device() & 63])

// calcul_tables(), LabQ2sRGB.c:130-160
static void calcul_tables(int range, std::vector<int> &Y2v, std::vector<float> &v2Y)
{
	Y2v.resize(range + 1);
	v2Y.resize(range);
	for (int i = 0; i < range; i++) {
		float f = (float) i / (range - 1);
		float v;

		if (f <= 0.0031308)
			v = 12.92F * f;
		else
			v = (1.0F + 0.055F) * powf(f, 1.0F / 2.4F) - 0.055F;

		Y2v[i] = rintf((range - 1) * v);
	}
	Y2v[range] = Y2v[range - 1];

	for (int i = 0; i < range; i++) {
		float f = (float) i / (range - 1);

		if (f <= 0.04045)
			v2Y[i] = f / 12.92F;
		else
			v2Y[i] = powf((f + 0.055F) / (1 + 0.055F), 2.4F);
	}
}

static void cbrt_table(std::vector<float> &cb)
{
	// table_init(), XYZ2Lab.c:92-106
	const int QUANT_ELEMENTS = 100000;
	cb.resize(QUANT_ELEMENTS);
	for (int i = 0; i < QUANT_ELEMENTS; i++) {
		float Y = (double) i / QUANT_ELEMENTS;

		if (Y < 0.008856)
			cb[i] = 7.787F * Y + (16.0F / 116.0F);
		else
			cb[i] = cbrtf(Y);
	}
}

void colour_tables_host(std::vector<float> &v2Y_8, std::vector<int> &Y2v_8, std::vector<float> &cbrt)
{
	calcul_tables(256, Y2v_8, v2Y_8);
	cbrt_table(cbrt);
}

// The tables of cbrt_exact.h for the calling thread's device: made from the cube-root table this
// host's libm produces, every entry checked to come out of cbrt_pair() bit for bit.  nullptr: the
// scheme does not fit this host's cbrtf (callers then read the table itself), or an upload failed.
const CbrtExact *cbrt_exact_tables()
{
	static std::mutex mutex;
	static CbrtExact by_device[64];
	static int state[64]; // 0 not tried, 1 ready, -1 unusable
	std::lock_guard<std::mutex> lock(mutex);
	const int dev = current_device() < 0 ? 0 : current_device() & 63;
	if (state[dev])
		return state[dev] > 0 ? &by_device[dev] : nullptr;
	state[dev] = -1;
	std::vector<float> cb;
	cbrt_table(cb);
	std::vector<CbrtBlockD> bd(CBRT_BLOCKS + 1);
	std::vector<CbrtBlockI> bi(CBRT_BLOCKS + 1);
	std::vector<unsigned int> res(CBRT_RES_WORDS, 0x55555555u); // residual 0 everywhere
	for (int k = 0; k <= CBRT_BLOCKS; k++) {
		bi[k].i0 = 0;
		bi[k].count = 0;
	}
	for (int i = 1; i < CBRT_N + 4096; i++) { // (one block past the table's last)
		const int k = (int) (cbrt_bits((float) i) >> 18) - CBRT_KEY0;
		if (k < 0 || k > CBRT_BLOCKS)
			continue;
		if (!bi[k].count)
			bi[k].i0 = i;
		bi[k].count++;
	}
	for (int k = 0; k <= CBRT_BLOCKS; k++) {
		if (!bi[k].count)
			return nullptr;
		bd[k].c0 = cbrt((double) bi[k].i0 / CBRT_N);
		bd[k].inv = 1.0 / bi[k].i0;
	}
	for (int i = CBRT_LINEAR; i < CBRT_N; i++) {
		const int k = (int) (cbrt_bits((float) i) >> 18) - CBRT_KEY0;
		if (k < 0 || k >= CBRT_BLOCKS)
			return nullptr;
		const long long r = (long long) cbrt_bits(cb[i]) - (long long) cbrt_predict(bd[k], bi[k], i);
		if (r < -1 || r > 1)
			return nullptr;
		res[i >> 4] = (res[i >> 4] & ~(3u << (2 * (i & 15)))) | ((unsigned int) (r + 1) << (2 * (i & 15)));
	}
	// every pair a kernel can ask for, against the table the reference would read
	{
		for (int pass = 0; pass < 2; pass++) {
		CbrtExact host = { bd.data(), bi.data(), res.data(), pass ? cb.data() : nullptr };
		for (int i = 0; i + 1 < CBRT_N; i++) {
			float t0, dt;
			cbrt_pair(host, i, &t0, &dt);
			const float want_dt = cb[i + 1] - cb[i];
			if (memcmp(&t0, &cb[i], 4) || memcmp(&dt, &want_dt, 4))
				return nullptr;
		}
		}
	}
	// the single-precision form, under the same two checks; left out (kernels take the double form)
	// when this host's cbrtf does not fit it
	std::vector<CbrtBlockF> bf(CBRT_BLOCKS + 1);
	std::vector<unsigned int> res32(CBRT_RES_WORDS, 0x55555555u);
	bool have32 = !getenv("VIPS_HIP_CBRT_F64");
	for (int k = 0; k <= CBRT_BLOCKS; k++) {
		bf[k].c0 = (float) bd[k].c0;
		bf[k].inv = (float) bd[k].inv;
	}
	for (int i = CBRT_LINEAR; i < CBRT_N && have32; i++) {
		const int k = (int) (cbrt_bits((float) i) >> 18) - CBRT_KEY0;
		const long long r = (long long) cbrt_bits(cb[i]) - (long long) cbrt_predict32(bf[k], i - bi[k].i0);
		if (r < -1 || r > 1)
			have32 = false;
		else
			res32[i >> 4] = (res32[i >> 4] & ~(3u << (2 * (i & 15)))) | ((unsigned int) (r + 1) << (2 * (i & 15)));
	}
	// (the first entry of a block must be the block's c0 itself: cbrt_pair32 reads it for the pair that straddles)
	for (int k = 1; k <= CBRT_BLOCKS && have32; k++)
		if (bi[k].i0 < CBRT_N && cbrt_predict32(bf[k], 0) != cbrt_bits(bf[k].c0))
			have32 = false;
	for (int pass = 0; pass < 2 && have32; pass++) {
		CbrtExact host = { bd.data(), bi.data(), res.data(), pass ? cb.data() : nullptr, bf.data(), res32.data() };
		for (int i = 0; i + 1 < CBRT_N && have32; i++) {
			float t0, dt;
			cbrt_pair32(host, i, &t0, &dt);
			const float want_dt = cb[i + 1] - cb[i];
			if (memcmp(&t0, &cb[i], 4) || memcmp(&dt, &want_dt, 4))
				have32 = false;
		}
	}
	if (getenv("VIPS_HIP_DEBUG_CBRT"))
		fprintf(stderr, "cbrt_exact_tables: the %s form\n", have32 ? "single-precision" : "double");
	CbrtExact &t = by_device[dev];
	t.bf = nullptr;
	t.res32 = nullptr;
	if (have32) {
		t.bf = (const CbrtBlockF *) upload(bf.data(), bf.size() * sizeof(CbrtBlockF));
		t.res32 = (const unsigned int *) upload(res32.data(), res32.size() * sizeof(unsigned int));
		if (!t.bf || !t.res32) {
			t.bf = nullptr;
			t.res32 = nullptr;
			vips_hip_error_clear();
		}
	}
	t.bd = (const CbrtBlockD *) upload(bd.data(), bd.size() * sizeof(CbrtBlockD));
	t.bi = (const CbrtBlockI *) upload(bi.data(), bi.size() * sizeof(CbrtBlockI));
	t.res = (const unsigned int *) upload(res.data(), res.size() * sizeof(unsigned int));
	t.lin = (const float *) upload(cb.data(), CBRT_LINEAR * sizeof(float));
	if (!t.bd || !t.bi || !t.res || !t.lin)
		return nullptr;
	state[dev] = 1;
	return &t;
}

// The tables of cbrt_quad.h for the calling thread's device, made from the cube-root table this host's libm
// produces: per block a least-squares quadratic through the exact cube roots, then the residuals and every pair
// checked by running cbq_pair() itself.  nullptr: the scheme does not fit this host's cbrtf, or an upload failed.
static const CbrtQuad *cbq_refused(int where)
{
	if (getenv("VIPS_HIP_DEBUG_CBRT"))
		fprintf(stderr, "cbrt_quad_tables: this host's cbrtf does not fit the scheme (check %d)\n", where);
	return nullptr;
}

const CbrtQuad *cbrt_quad_tables()
{
	static std::mutex mutex;
	static CbrtQuad by_device[64];
	static int state[64]; // 0 not tried, 1 ready, -1 unusable
	std::lock_guard<std::mutex> lock(mutex);
	const int dev = current_device() < 0 ? 0 : current_device() & 63;
	if (state[dev])
		return state[dev] > 0 ? &by_device[dev] : nullptr;
	state[dev] = -1;
	if (getenv("VIPS_HIP_NO_CBRT_QUAD"))
		return cbq_refused(1);
	std::vector<float> cb;
	cbrt_table(cb);
	std::vector<CbqBlock> blk(CBQ_BLOCKS);
	std::vector<int> first(CBQ_BLOCKS, -1), count(CBQ_BLOCKS, 0);
	for (int i = 0; i < CBQ_N; i++) {
		const int k = cbq_key((float) (i + CBQ_SHIFT));
		if (k < 0 || k >= CBQ_BLOCKS)
			return cbq_refused(2);
		if (first[k] < 0)
			first[k] = i;
		count[k]++;
	}
	for (int k = 0; k < CBQ_BLOCKS; k++) {
		CbqBlock &q = blk[k];
		q.c0 = q.c1 = q.c2 = q.next = 0.0f;
		if (first[k] < 0)
			continue; // (a key no integer has)
		const int i0 = first[k], n = count[k];
		q.c0 = cb[i0];
		q.next = i0 + n < CBQ_N ? cb[i0 + n] : cb[CBQ_N - 1];
		if (n >= 2) {
			// least squares of T[i0 + j] - c0 = c1 j + c2 j^2 over the block (c2 = 0 for two entries)
			double s11 = 0, s12 = 0, s22 = 0, r1 = 0, r2 = 0;
			for (int j = 1; j < n; j++) {
				const double y = (double) cb[i0 + j] - (double) q.c0, x = j, x2 = x * x;
				s11 += x * x;
				s12 += x * x2;
				s22 += x2 * x2;
				r1 += x * y;
				r2 += x2 * y;
			}
			if (n == 2) {
				q.c1 = (float) (r1 / s11);
			}
			else {
				const double det = s11 * s22 - s12 * s12;
				q.c1 = (float) ((r1 * s22 - r2 * s12) / det);
				q.c2 = (float) ((r2 * s11 - r1 * s12) / det);
			}
		}
	}
	// residuals: a signed 2-bit field + the block's bias (the lowest bit of c2, which takes part in the
	// prediction: set first, then measured)
	std::vector<unsigned int> res(CBQ_RES_WORDS, 0u);
	for (int k = 0; k < CBQ_BLOCKS; k++) {
		if (first[k] < 0)
			continue;
		const int i0 = first[k], n = count[k];
		bool done = false;
		for (unsigned int bias = 0; bias < 2 && !done; bias++) {
			CbqBlock q = blk[k];
			q.c2 = cbq_float((cbq_bits(q.c2) & ~1u) | bias);
			bool ok = true;
			for (int j = 0; j < n && ok; j++) {
				const long long r = (long long) cbq_bits(cb[i0 + j]) - (long long) cbq_bits(cbq_predict(q, (float) j)) - (long long) bias;
				ok = r >= -2 && r <= 1 && (j > 0 || r + (long long) bias == 0);
			}
			if (!ok)
				continue;
			blk[k] = q;
			for (int j = 0; j < n; j++) {
				const int i = i0 + j;
				const long long r = (long long) cbq_bits(cb[i]) - (long long) cbq_bits(cbq_predict(q, (float) j)) - (long long) bias;
				res[i >> 4] |= ((unsigned int) r & 3u) << (2 * (i & 15));
			}
			done = true;
		}
		if (!done)
			return cbq_refused(100 + k);
	}
	// every pair a kernel can ask for, against the table the reference would read
	for (int i = 0; i + 1 < CBQ_N; i++) {
		float t0, dt;
		cbq_pair(blk.data(), res.data(), i, (float) i, &t0, &dt);
		const float want_dt = cb[i + 1] - cb[i];
		if (memcmp(&t0, &cb[i], 4) || memcmp(&dt, &want_dt, 4))
			return cbq_refused(4);
	}
	if (getenv("VIPS_HIP_DEBUG_CBRT"))
		fprintf(stderr, "cbrt_quad_tables: every pair checked\n");
	CbrtQuad &t = by_device[dev];
	t.blk = (const CbqBlock *) upload(blk.data(), blk.size() * sizeof(CbqBlock));
	t.res = (const unsigned int *) upload(res.data(), res.size() * sizeof(unsigned int));
	if (!t.blk || !t.res) {
		vips_hip_error_clear();
		return cbq_refused(5);
	}
	state[dev] = 1;
	return &t;
}

// The tables of the calling thread's device, made and uploaded on first use, copied to *out: the one way the other
// files of the colour path come by them.  0 on success
int colour_tables(ColourTables *out)
{
	std::lock_guard<std::mutex> lock(g_tables_mutex);
	if (g_tables.cbrt) {
		*out = g_tables;
		return 0;
	}
	std::vector<int> Y2v;
	std::vector<float> v2Y;
	calcul_tables(256, Y2v, v2Y);
	g_tables.Y2v_8 = (int *) upload(Y2v.data(), Y2v.size() * sizeof(int));
	g_tables.v2Y_8 = (float *) upload(v2Y.data(), v2Y.size() * sizeof(float));
	calcul_tables(65536, Y2v, v2Y);
	g_tables.Y2v_16 = (int *) upload(Y2v.data(), Y2v.size() * sizeof(int));
	g_tables.v2Y_16 = (float *) upload(v2Y.data(), v2Y.size() * sizeof(float));
	std::vector<float> cb;
	cbrt_table(cb);
	float *cbrt = (float *) upload(cb.data(), cb.size() * sizeof(float));
	if (!g_tables.Y2v_8 || !g_tables.v2Y_8 || !g_tables.Y2v_16 || !g_tables.v2Y_16 || !cbrt)
		return -1;
	g_tables.cbrt = cbrt;
	*out = g_tables;
	return 0;
}

} // namespace vh
