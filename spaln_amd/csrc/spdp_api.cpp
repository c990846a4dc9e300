// spdp_api.cpp -- host side of libspdp_hip.so: the extern "C" surface declared in
// include/spdp.h.  Packs problems into the HBM layout of spdp_dev.h and launches
// the sweeps of spdp_kernels.hip; the reference's dispatch logic around the
// engines (Aln2s1::lspS_ng & co., src/fwd2s1.cc:1667-1897) lives in
// spdp_host.cpp.  There is no CPU compute path: without a HIP device
// spdp_create() fails.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/spdp.h"
#include "spdp_dev.h"
#include "spdp_internal.h"
#include "spdp_ladder.h"

// ---- small helpers --------------------------------------------------------------
void spdp_stripe(const SpdpProblem* p, int sh, SpdpWindow* w)
{   // stripe(), src/aln2.cc:156-176 (cmode 3)
    ladder::stripe<1>(p->a_left, p->a_right, p->b_left, p->b_right, sh, w);
}

int64_t spdp_cells_w(int a_left, int a_right, int b_left, int b_right, const SpdpWindow& w)
{   // cells visited by the reference loops, src/fwd2s1.cc:249-256:
    //   sum over m in (a_left, a_right] of max(0, min(m + up + 1, b_right) - max(m + lw, b_left)),
    // evaluated piecewise (both clamps switch once along m)
    auto seg = [&](int64_t m0, int64_t m1, bool hi_clamped, bool lo_clamped) -> int64_t {
        if (m1 < m0) return 0;                           // rows m0 .. m1 inclusive
        const int64_t cnt = m1 - m0 + 1, sm = (m0 + m1) * cnt / 2;
        // width(m) = (hi_clamped ? b_right : m + up + 1) - (lo_clamped ? b_left : m + lw)
        int64_t tot = 0;
        tot += hi_clamped ? (int64_t) b_right * cnt : sm + (int64_t) (w.up + 1) * cnt;
        tot -= lo_clamped ? (int64_t) b_left * cnt : sm + (int64_t) w.lw * cnt;
        return tot;
    };
    const int64_t mh = (int64_t) b_right - w.up - 1;     // m >= mh: upper end clamped to b_right
    const int64_t ml = (int64_t) b_left - w.lw;          // m <= ml: lower end clamped to b_left
    int64_t c = 0;
    int64_t cuts[4] = {a_left + 1, std::min<int64_t>(std::max<int64_t>(mh, a_left + 1), a_right + 1),
                       std::min<int64_t>(std::max<int64_t>(ml + 1, a_left + 1), a_right + 1), a_right + 1};
    std::sort(cuts, cuts + 4);
    for (int i = 0; i < 3; ++i) {
        const int64_t m0 = cuts[i], m1 = cuts[i + 1] - 1;
        if (m1 < m0) continue;
        const bool hi = m0 >= mh, lo = m1 <= ml;
        // within a segment both flags are constant; widths are linear, so a negative width can only
        // occur over a whole prefix/suffix -- fall back to the exact loop in that rare case
        const int64_t w0 = (hi ? b_right : m0 + w.up + 1) - (lo ? b_left : m0 + w.lw);
        const int64_t w1 = (hi ? b_right : m1 + w.up + 1) - (lo ? b_left : m1 + w.lw);
        if (w0 >= 0 && w1 >= 0) c += seg(m0, m1, hi, lo);
        else
            for (int64_t m = m0; m <= m1; ++m) {
                const int64_t n1 = std::max<int64_t>(m + w.lw, b_left), n9 = std::min<int64_t>(m + w.up + 1, b_right);
                if (n9 > n1) c += n9 - n1;
            }
    }
    return c;
}

int64_t spdp_cells(const SpdpProblem* p, const SpdpWindow* w)
{
    return spdp_cells_w(p->a_left, p->a_right, p->b_left, p->b_right, *w);
}

RunItem spdp_item_of(const SpdpProblem& p, int parent, int sh)
{
    RunItem it;
    it.parent = parent;
    it.a_left = p.a_left; it.a_right = p.a_right; it.b_left = p.b_left; it.b_right = p.b_right;
    it.a_exgl = p.a_exgl; it.a_exgr = p.a_exgr; it.b_exgl = p.b_exgl; it.b_exgr = p.b_exgr;
    ladder::stripe<1>(p.a_left, p.a_right, p.b_left, p.b_right, sh, &it.w);
    it.n_im = 0;
    return it;
}

// ---- context ----------------------------------------------------------------------
SpdpContext* spdp_create(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fprintf(stderr, "spdp_create: no HIP device (this library has no CPU path)\n");
        return nullptr;
    }
    if (device < 0 || device >= ndev) return nullptr;
    SpdpContext* ctx = new SpdpContext();
    ctx->device = device;
    // the main stream carries the latency-bound launches (linear-space rounds, slab tracebacks): highest priority;
    // the side stream (a big forward sweep beside them) the lowest
    int prio_lo = 0, prio_hi = 0;
    if (hipSetDevice(device) != hipSuccess) { delete ctx; return nullptr; }
    (void) hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (hipStreamCreateWithPriority(&ctx->stream, hipStreamDefault, prio_hi) != hipSuccess) {
        delete ctx;
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        ctx->n_cu = prop.multiProcessorCount;
        ctx->name = std::string(prop.name) + " " + prop.gcnArchName;
    }
    if (ctx->n_cu <= 0) ctx->n_cu = 256;
    (void) hipEventCreate(&ctx->ev0);
    (void) hipEventCreate(&ctx->ev1);
    if (hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, prio_lo) != hipSuccess) ctx->stream2 = nullptr;
    (void) hipEventCreate(&ctx->ev2);
    (void) hipEventCreate(&ctx->ev3);
    return ctx;
}

void* DevPool::get(int slot, size_t bytes)
{
    if (bytes < 256) bytes = 256;
    if (cap[slot] >= bytes) return ptr[slot];
    if (ptr[slot]) (void) hipFree(ptr[slot]);
    ptr[slot] = nullptr; cap[slot] = 0;
    size_t want = bytes + bytes / 8;                    // head-room: batches of one run vary a little
    if (hipMalloc(&ptr[slot], want) != hipSuccess) {
        if (hipMalloc(&ptr[slot], bytes) != hipSuccess) return nullptr;
        want = bytes;
    }
    cap[slot] = want;
    return ptr[slot];
}

void DevPool::release()
{
    for (int i = 0; i < N_SLOTS; ++i) { if (ptr[i]) (void) hipFree(ptr[i]); ptr[i] = nullptr; cap[i] = 0; }
}

thread_local bool t_lane_copies = false;         // spdp_internal.h, spdp_copy_sync

// lane i of a context: lane 0 is the context itself, the others are contexts of their own (stream, side stream, events,
// pools, signal words, staging) on the same device, created on first use and owned by the parent.  Two lanes therefore
// never touch one pool slot, and a lane's runs are waited for before a slot is taken again (DevRun::sync / release).
// DevPool::get still frees and allocates when a slot has to grow, which waits for the whole device: the first call after
// a change of plan stalls there behind the other lane's sweep, later calls do not.
SpdpContext* spdp_lane(SpdpContext* ctx, int i)
{
    if (i <= 0) return ctx;
    while ((int) ctx->lanes.size() < i) {
        SpdpContext* l = spdp_create(ctx->device);
        if (!l) return nullptr;
        ctx->lanes.push_back(l);
    }
    return ctx->lanes[i - 1];
}

void spdp_destroy(SpdpContext* ctx)
{
    if (!ctx) return;
    for (SpdpContext* l : ctx->lanes) spdp_destroy(l);
    ctx->lanes.clear();
    (void) hipSetDevice(ctx->device);
    for (DevPool& p : ctx->pool) p.release();
    for (int k = 0; k < 3; ++k) if (ctx->stage_ptr[k]) (void) hipHostFree(ctx->stage_ptr[k]);
    if (ctx->d_started) (void) hipFree(ctx->d_started);
    if (ctx->sig_host) (void) hipHostFree(ctx->sig_host);
    (void) hipEventDestroy(ctx->ev0);
    (void) hipEventDestroy(ctx->ev1);
    (void) hipEventDestroy(ctx->ev2);
    (void) hipEventDestroy(ctx->ev3);
    if (ctx->stream2) (void) hipStreamDestroy(ctx->stream2);
    (void) hipStreamDestroy(ctx->stream);
    delete ctx;
}

int SpdpContext::start_signal()
{
    SpdpContext* ctx = this;
    if (d_started && sig_host_dev) return 0;
    if (!d_started) HIPCHK(hipMalloc((void**) &d_started, 256));
    if (!sig_host) {
        HIPCHK(hipHostMalloc((void**) &sig_host, 256, hipHostMallocMapped | hipHostMallocCoherent));
        *sig_host = 0;
    }
    HIPCHK(hipHostGetDevicePointer((void**) &sig_host_dev, sig_host, 0));
    return 0;
}

void* SpdpContext::staging(int k, size_t bytes)
{
    if (bytes <= stage_cap[k]) return stage_ptr[k];
    if (stage_ptr[k]) (void) hipHostFree(stage_ptr[k]);
    stage_ptr[k] = nullptr; stage_cap[k] = 0;
    const size_t want = bytes + bytes / 8;
    if (hipHostMalloc(&stage_ptr[k], want, hipHostMallocDefault) != hipSuccess) { stage_ptr[k] = nullptr; return nullptr; }
    stage_cap[k] = want;
    return stage_ptr[k];
}

// the staging ring of spdp_internal.h.  The calling thread issues the copies and never packs: a packer may wait on `copied`, which
// only the calling thread advances
int spdp_upload_ring(SpdpContext* ctx, const std::vector<int64_t>& off, int64_t tot, int64_t grp_positions,
                     std::vector<StagedStream>& st, const std::function<void(int i, int64_t at)>& pack)
{
    const int n = (int) off.size(), ring = 4;
    std::vector<int> grp_first, grp_of(n);
    int64_t slot_cap = 1, acc = 0;
    for (int i = 0; i < n; ++i) {
        if (i == 0 || acc >= grp_positions) { grp_first.push_back(i); acc = 0; }
        grp_of[i] = (int) grp_first.size() - 1;
        acc += (i + 1 < n ? off[i + 1] : tot) - off[i];
        slot_cap = std::max(slot_cap, acc);
    }
    for (StagedStream& s : st)
        if (!(s.host = ctx->staging(s.slot, (size_t) slot_cap * ring * s.bytes))) { ctx->err = "out of pinned host memory"; return -1; }
    const int n_grp = (int) grp_first.size();
    std::atomic<int> copied{0};                         // groups whose copy has left the staging
    std::vector<std::atomic<int>> grp_done(n_grp);      // problems packed, per group
    for (auto& g : grp_done) g.store(0);
    std::atomic<int> next_prob{0};
    auto packer = [&] {
        for (int i; (i = next_prob.fetch_add(1)) < n; ) {
            const int g = grp_of[i];
            while (copied.load(std::memory_order_acquire) < g - ring + 1) std::this_thread::yield();
            pack(i, (int64_t) (g % ring) * slot_cap + (off[i] - off[grp_first[g]]));
            grp_done[g].fetch_add(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> th;
    for (int t = 0, nt = std::max(1, std::min(spdp_host_cpus(), n)); t < nt; ++t) th.emplace_back(packer);
    hipError_t ce = hipSuccess;
    std::vector<hipEvent_t> left((size_t) ring, nullptr);
    for (int k = 0; k < ring && ce == hipSuccess && n_grp > ring; ++k) ce = hipEventCreateWithFlags(&left[k], hipEventDisableTiming);
    for (int g = 0; g < n_grp && ce == hipSuccess; ++g) {
        const int first = grp_first[g], last = g + 1 < n_grp ? grp_first[g + 1] : n;
        while (grp_done[g].load(std::memory_order_acquire) < last - first) std::this_thread::yield();
        const int64_t c0 = off[first], c1 = last < n ? off[last] : tot, s0 = (int64_t) (g % ring) * slot_cap;
        for (const StagedStream& s : st)
            if (ce == hipSuccess)
                ce = hipMemcpyAsync((char*) s.dev + c0 * s.bytes, (char*) s.host + s0 * s.bytes, (size_t) (c1 - c0) * s.bytes,
                                    hipMemcpyHostToDevice, ctx->stream);
        if (n_grp > ring) {                             // (a call of up to four groups never waits: every group has its slot)
            if (ce == hipSuccess) ce = hipEventRecord(left[g % ring], ctx->stream);
            if (ce == hipSuccess && g >= 1) { ce = hipEventSynchronize(left[(g - 1) % ring]); copied.store(g, std::memory_order_release); }
        }
    }
    copied.store(INT32_MAX, std::memory_order_release);                   // (on an error too: no packer may wait for ever)
    for (std::thread& t : th) t.join();
    const hipError_t se = hipStreamSynchronize(ctx->stream);              // the staging is the context's: one upload at a time
    for (hipEvent_t e : left) if (e) (void) hipEventDestroy(e);
    if (ce == hipSuccess) ce = se;
    if (ce != hipSuccess) { ctx->err = std::string("column record upload: ") + hipGetErrorString(ce); return -1; }
    return 0;
}

int spdp_upload_cip(SpdpContext* ctx, int n, const std::function<const int32_t*(int i, size_t& len)>& row, std::vector<int32_t>& off,
                    void** d)
{
    off.assign(n, -1);
    std::vector<int32_t> h;
    for (int i = 0; i < n; ++i) {
        size_t len = 0;
        if (const int32_t* r = row(i, len)) { off[i] = (int32_t) h.size(); h.insert(h.end(), r, r + len); }
    }
    if (h.empty()) return 0;
    HIPCHK(hipMalloc(d, h.size() * sizeof(int32_t)));
    HIPCHK(hipMemcpy(*d, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

const char* spdp_last_error(const SpdpContext* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int spdp_device_name(const SpdpContext* ctx, char* buf, int buflen)
{
    if (!ctx || !buf || buflen <= 0) return -1;
    snprintf(buf, buflen, "%s (%d CUs)", ctx->name.c_str(), ctx->n_cu);
    return 0;
}

// ---- resident inputs ----------------------------------------------------------------
static void to_dev_scoring(const SpdpScoring* sc, DevScoring* d)
{
    memset(d, 0, sizeof *d);
    d->mtx_dim = sc->mtx_dim;
    d->gop = sc->gop; d->gep = sc->gep;
    d->spj = sc->spj; d->llmt = sc->llmt;
    d->nquant = std::max(1, std::min(sc->nquant, SPDP_MAX_QUANT));
    d->local = sc->local ? 1 : 0;
    for (int j = 0; j < SPDP_MAX_QUANT; ++j) { d->qm_len[j] = sc->qm_len[j]; d->qm_pen[j] = sc->qm_pen[j]; }
    for (int i = 1; i < sc->mtx_dim && i < 32; ++i)         // row / column 0 stay zero
        for (int j = 1; j < sc->mtx_dim && j < 32; ++j)
            d->mtx[i * 32 + j] = sc->mtx[i * sc->mtx_dim + j];
}

void DevStore::release()
{
    if (!ctx) return;
    (void) hipSetDevice(ctx->device);
    if (d_sc) (void) hipFree(d_sc);
    if (d_a) (void) hipFree(d_a);
    if (d_cols) (void) hipFree(d_cols);
    if (d_aux) (void) hipFree(d_aux);
    if (d_intpen) (void) hipFree(d_intpen);
    if (d_ipen_runs) (void) hipFree(d_ipen_runs);
    d_ipen_runs = nullptr;
    if (d_cip) (void) hipFree(d_cip);
    d_sc = d_a = d_cols = d_aux = d_intpen = d_cip = nullptr;
}

int DevStore::upload(SpdpContext* c, const SpdpScoring* scp, const SpdpProblem* probs, int n)
{
    ctx = c; sc = *scp; n_parents = n;
    (void) hipSetDevice(ctx->device);
    // double affine gaps (Noll = 3, -yl3): forwardS_ng / hirschbergS_ng / scorealoneS_ng (the -A0 engines, spdp_rowwave<., ., ., DAGP>,
    // spdp_rowwave_udh<., DAGP>); the -A1 / -A2 / -A3 engines and the seeded walk's cut range refuse it (DevRun::check)
    if (sc.noll != 2 && !(sc.noll == 3 && (sc.scalar_engines == 1 || sc.scalar_engines == 2))) {
        ctx->err = "double affine gaps (Noll = 3) are built for the -A0 and -A1 engines (SpdpScoring.scalar_engines = 1 / 2); Noll must be 2 or 3";
        return -1;
    }
    // GapPenalty(1) of the first column is BasicGOP + BasicGEP only while codonk1 >= 1 (src/aln.h:275-282); a caller that leaves
    // the field 0 would silently get scores that are not the reference's
    if (sc.noll == 3 && sc.codonk1 < 1) { ctx->err = "Noll = 3 needs SpdpScoring.codonk1 >= 1 (alprm2.k1 of the reference)"; return -1; }
    if (sc.mtx_dim < 1 || sc.mtx_dim > 32) { ctx->err = "mtx_dim out of range"; return -1; }
    a_off.resize(n); col_off.resize(n); a_len.resize(n); b_len.resize(n);
    int64_t a_tot = 0, col_tot = 0;
    for (int i = 0; i < n; ++i) {
        const SpdpProblem& p = probs[i];
        if (p.a_right > p.a_len || p.b_right > p.b_len || p.a_left < 0 || p.b_left < 0 ||
            p.a_right < p.a_left || p.b_right < p.b_left) { ctx->err = "bad problem ranges"; return -1; }
        a_len[i] = p.a_len; b_len[i] = p.b_len;
        a_off[i] = a_tot; a_tot += ((int64_t) p.a_len + 15) & ~15ll;
        col_off[i] = col_tot; col_tot += (int64_t) p.b_len + 1 + SPDP_COL_PAD;
    }
    std::vector<uint8_t> ha(std::max<int64_t>(a_tot, 16), 0);
    // signals: either every problem brings sig5 / sig3 (then also cano5 / cano3 / dinc for the exact engines), or none
    // does and SpdpScoring::sigmodel says how to compute them from the codes -- on the device (spdp_signals.hip)
    int n_sig = 0;
    for (int i = 0; i < n; ++i) n_sig += (probs[i].sig5 && probs[i].sig3) ? 1 : 0;
    const bool dev_sig = n > 0 && n_sig == 0 && sc.sigmodel;
    if (n_sig != n && !dev_sig) {
        ctx->err = n_sig ? "sig5 / sig3 missing for part of the batch" : "sig5 / sig3 missing and no SpdpScoring::sigmodel";
        return -1;
    }
    has_exact = sc.intpen && sc.intpen_len > 0;
    for (int i = 0; i < n && has_exact && !dev_sig; ++i)
        if (!probs[i].cano5 || !probs[i].cano3 || !probs[i].dinc) has_exact = false;
    int max_s5 = INT32_MIN, max_s3 = INT32_MIN;
    for (int i = 0; i < n; ++i) memcpy(ha.data() + a_off[i], probs[i].a, probs[i].a_len);
    HIPCHK(hipMalloc(&d_cols, 2 * std::max<int64_t>(col_tot, 1) * sizeof(int32_t)));
    if (has_exact) HIPCHK(hipMalloc(&d_aux, 2 * std::max<int64_t>(col_tot, 1)));
    if (dev_sig) {
        // codes only over PCIe (1 B per position instead of 8 + 2): base i of problem p at hb[col_off + i]
        std::vector<uint8_t> hb(std::max<int64_t>(col_tot, 16), 0);
        std::vector<SigJob> jobs(n);
        for (int i = 0; i < n; ++i) {
            memcpy(hb.data() + col_off[i], probs[i].b, probs[i].b_len);
            SigJob& J = jobs[i];
            J.b_off = J.col_off = col_off[i]; J.out_off = 0; J.pad = 0;
            J.b_len = probs[i].b_len; J.left = probs[i].b_left; J.right = probs[i].b_right;
            if (probs[i].exin_left || probs[i].exin_right) {      // the range the reference's Exinon covers, not the call's sub-range
                if (probs[i].exin_left < 0 || probs[i].exin_right > probs[i].b_len || probs[i].exin_left > probs[i].b_left ||
                    probs[i].exin_right < probs[i].b_right) { ctx->err = "exin_left / exin_right must enclose b_left / b_right"; return -1; }
                J.left = probs[i].exin_left; J.right = probs[i].exin_right;
            }
        }
        void* d_b = nullptr;
        HIPCHK(hipMalloc(&d_b, hb.size()));
        hipError_t e = hipMemcpyAsync(d_b, hb.data(), hb.size(), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_cols, 0, 2 * std::max<int64_t>(col_tot, 1) * sizeof(int32_t), ctx->stream);
        if (e == hipSuccess && has_exact) e = hipMemsetAsync(d_aux, 0, 2 * std::max<int64_t>(col_tot, 1), ctx->stream);
        int rc = -1;
        if (e == hipSuccess) {
            SignalArgs A;
            memset(&A, 0, sizeof A);
            A.codes = (const uint8_t*) d_b;
            A.cols = (int2*) d_cols; A.aux = has_exact ? (uchar2*) d_aux : nullptr;
            A.ipen = sc.ipen; A.spj = sc.spj;
            rc = spdp_signals_run(ctx, sc.sigmodel, jobs, A, &max_s5, &max_s3);
        } else {
            ctx->err = std::string("signal upload: ") + hipGetErrorString(e);
        }
        (void) hipFree(d_b);
        if (rc) return -1;
    } else {
        // column records (8 B per genomic position) and class bytes, packed by all host cores into pinned staging memory the context
        // keeps (a 10 k batch is ~1 GB: one thread and pageable memory took 430 ms, 40 % of a step) and copied in groups of ~8 M
        // positions under the packing of the next ones (a map + align call holds 5 * 10^8 positions: 5 GB of pinned memory when
        // every group had a place of its own)
        std::vector<StagedStream> st = {{0, d_cols, 2 * sizeof(int32_t)}};
        if (has_exact) st.push_back({1, d_aux, 2});
        std::vector<int> p_s5(n, INT32_MIN), p_s3(n, INT32_MIN);
        if (spdp_upload_ring(ctx, col_off, col_tot, 8 << 20, st, [&](int i, int64_t at) {
                const SpdpProblem& p = probs[i];
                if (has_exact) {
                    uint8_t* x = (uint8_t*) st[1].host + 2 * at;
                    for (int nn = 0; nn <= p.b_len; ++nn, x += 2) {
                        x[0] = (p.cano5[nn] ? 1 : 0) | (p.cano3[nn] ? 2 : 0);
                        x[1] = p.dinc[nn];
                    }
                    memset(x, 0, 2 * SPDP_COL_PAD);
                }
                int32_t* cr = (int32_t*) st[0].host + 2 * at;
                int m5 = INT32_MIN, m3 = INT32_MIN;
                for (int nn = 0; nn <= p.b_len; ++nn, cr += 2) {
                    const uint16_t s5 = (uint16_t) (int16_t) (p.sig5[nn] + sc.ipen);
                    const uint16_t s3 = (uint16_t) p.sig3[nn];
                    cr[0] = sc.spj ? (int32_t) ((uint32_t) s5 | ((uint32_t) s3 << 16)) : 0;
                    m5 = std::max(m5, (int) (int16_t) s5); m3 = std::max(m3, (int) (int16_t) s3);
                    cr[1] = nn > 0 ? p.b[nn - 1] : 0;
                }
                memset(cr, 0, 2 * SPDP_COL_PAD * sizeof(int32_t));
                p_s5[i] = m5; p_s3[i] = m3;
            })) return -1;
        for (int i = 0; i < n; ++i) { max_s5 = std::max(max_s5, p_s5[i]); max_s3 = std::max(max_s3, p_s3[i]); }
    }
    sc.sigmodel = nullptr;                                   // the caller's model is not ours to keep
    this->max_s5 = max_s5; this->max_s3 = max_s3;
    // bounds for the fp32 sweeps (DevRun::build): best substitution score, best net gain of one intron
    fp_maxpos = 1;
    for (int i = 0; i < sc.mtx_dim * sc.mtx_dim; ++i) fp_maxpos = std::max(fp_maxpos, (int) sc.mtx[i]);
    {
        int max_pen = INT32_MIN;
        for (int j = 0; j < std::max(1, std::min(sc.nquant, SPDP_MAX_QUANT)); ++j) max_pen = std::max(max_pen, (int) sc.qm_pen[j]);
        fp_gain = (sc.spj && max_s5 > INT32_MIN) ? std::max(0, max_s5 + max_s3 + max_pen) : 0;
    }
    // conserved-intron bonuses of the queries that carry them (SpdpProblem::cip), one row of a_len + 1 ints each
    if (spdp_upload_cip(ctx, n, [&](int i, size_t& len) { len = (size_t) probs[i].a_len + 1; return probs[i].cip; }, cip_off, &d_cip)) return -1;
    DevScoring hsc;
    to_dev_scoring(&sc, &hsc);
    HIPCHK(hipMalloc(&d_sc, sizeof(DevScoring)));
    HIPCHK(hipMalloc(&d_a, ha.size()));
    HIPCHK(hipMemcpyAsync(d_sc, &hsc, sizeof hsc, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_a, ha.data(), ha.size(), hipMemcpyHostToDevice, ctx->stream));
    if (has_exact) {
        HIPCHK(hipMalloc(&d_intpen, sizeof(int16_t) * sc.intpen_len));
        HIPCHK(hipMemcpyAsync(d_intpen, sc.intpen, sizeof(int16_t) * sc.intpen_len, hipMemcpyHostToDevice, ctx->stream));
        std::vector<int16_t> runs(SPDP_IPR_WORDS);
        if (spdp_intpen_runs(sc.intpen, sc.intpen_len, runs.data())) {
            HIPCHK(hipMalloc(&d_ipen_runs, sizeof(int16_t) * runs.size()));
            HIPCHK(hipMemcpy(d_ipen_runs, runs.data(), sizeof(int16_t) * runs.size(), hipMemcpyHostToDevice));
        }
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- one sweep over a list of items ---------------------------------------------------
// the 16-column blocks of traceback codes that stripe s of a forward sweep writes
static int stripe_blocks(const RunItem& it, int s)
{
    const int ml = it.a_left + s * SPDP_NELEM, j9 = std::min(SPDP_NELEM, it.a_right - ml);
    const int n_start = std::max(it.b_left, it.w.lw + ml);
    const int n9 = std::min(it.b_right, it.w.up + (ml + j9) + 1) + j9;
    return (std::max(0, n9 + 1 - n_start) + 15) >> 4;
}
static int stripes_of(const DevProblem& P) { return (P.a_right - P.a_left + SPDP_NELEM - 1) / SPDP_NELEM; }

// buffers belong to pool(); a run abandoned in flight (an error elsewhere in the batch) is waited for so
// that its pool can be reused
void DevRun::release() { if (in_flight && ctx) { (void) hipStreamSynchronize(strm()); in_flight = false; } }

#define POOLGET(dst, slot, bytes) do { if (!((dst) = take((slot), (size_t) (bytes)))) return -1; } while (0)
void* DevRun::take(int slot, size_t bytes) { void* p = pool().get(slot, bytes); if (!p) ctx->err = "out of device memory"; return p; }

bool spdp_intpen_runs(const int16_t* intpen, int len, int16_t* out)
{
    if (len <= SPDP_IPR_BASE) {                         // nothing beyond the LDS table: one run
        if (len <= 0) return false;
        memset(out, 0, sizeof(int16_t) * SPDP_IPR_WORDS);
        uint16_t* st = (uint16_t*) out;
        st[0] = SPDP_IPR_BASE; st[1] = 65535;
        out[SPDP_IPR_RUNS + 1] = intpen[len - 1];
        return true;
    }
    if (len > 65536) return false;
    uint16_t* start = (uint16_t*) out;
    int16_t* val = out + SPDP_IPR_RUNS + 1;
    uint8_t* span = (uint8_t*) (out + SPDP_IPR_RUNS + 1 + SPDP_IPR_RUNS);
    int nr = 0;
    start[0] = SPDP_IPR_BASE; val[0] = intpen[SPDP_IPR_BASE];
    for (int i = SPDP_IPR_BASE + 1; i < len; ++i)
        if (intpen[i] != intpen[i - 1]) {
            if (++nr >= SPDP_IPR_RUNS) return false;
            start[nr] = (uint16_t) i; val[nr] = intpen[i];
        }
    for (int j = nr + 1; j <= SPDP_IPR_RUNS; ++j) start[j] = 65535;
    for (int j = nr + 1; j < SPDP_IPR_RUNS; ++j) val[j] = val[nr];
    int j = 0;
    for (int b = 0; b < SPDP_IPR_SPANS; ++b) {
        const int lo = SPDP_IPR_BASE + 64 * b, hi = lo + 63;
        while (j < nr && (int) start[j + 1] <= lo) ++j;
        span[b] = (uint8_t) j;
        if (j + 2 <= nr && (int) start[j + 2] <= hi) return false;      // two steps inside one span
    }
    return true;
}

// Vmf record budget of one forwardS_ng / forwardS1 call.  A record is written where a diagonal run starts and twice per
// accepted intron: on real alignments a few per row.  The budget is one record per two band cells (the band, not the
// bounding rectangle), at least 64 per row; a call that outgrows it reports so (n_skl = -3) and is run again with
// vmf_scale x 8 by the ladder -- the old "two per cell of the rectangle" made batches of slabs run in dozens of groups.
int64_t vmf_capacity(int64_t rows, int64_t cols, int64_t width, int64_t scale)
{
    const int64_t band = rows * std::min(cols, width);
    const int64_t full = 2 * rows * cols + 64;
    return std::min(full, std::max(band / 2, 64 * rows) * scale + 64);
}

// what the engine cannot run at all (the callers and the tests know these messages)
int DevRun::check()
{
    const RunTraits& T = traits();
    if (T.family != FAM_WIP && !store->has_exact) {
        ctx->err = "scalar exact engine needs intpen / t53 in SpdpScoring and cano5 / cano3 / dinc per problem";
        return -1;
    }
    if (store->sc.noll == 3 && !(T.family == FAM_A0 || (T.family == FAM_A1 && T.kind != KIND_UDH))) {
        // (-A1: scoreonlyS1 / forwardS1 since round 5; the reference's own hirschbergS1 is not usable under -yl3 -- it never lets
        //  the second vertical gap reach H across an intermediate row -- so there is no result to be identical with)
        ctx->err = flavour == RUN_A1_UDH ? "double affine gaps (Noll = 3) under -A1: the linear-space engine (hirschbergS1) is undefined in the reference; "
                                        "raise SpdpScoring.max_vmf_space so that the traceback branch is taken"
                                      : "double affine gaps (Noll = 3): only the -A0 and -A1 engines are built";
        return -1;
    }
    return 0;
}

// one item's share of the three work buffers: ints (x RunTraits::bw) of bnd, traceback bytes or Vmf records of tb, ints of imd
struct ItemShare { int64_t work, tb, imd; };
static ItemShare item_share(const RunTraits& T, const RunItem& it, int noll)
{
    const int64_t width = it.w.width, buf = width + 2 * SPDP_NELEM, rows = it.a_right - it.a_left;
    const int64_t n_im = T.rows() ? it.n_im : 0;
    const int64_t cap = T.vmf ? vmf_capacity(rows + 1, it.b_right - it.b_left + 1, width, it.vmf_scale) : 0;
    switch (T.family) {
    case FAM_WIP: {                 // the boundary of one stripe; forward: a 256-byte block of codes per 16 columns of a stripe
        int64_t tb = 0;
        if (T.kind == KIND_FORWARD)
            for (int s = 0; s < (rows + SPDP_NELEM - 1) / SPDP_NELEM; ++s) tb += 256ll * stripe_blocks(it, s);
        return {buf + SPDP_BND_PAD, tb, n_im * 4 * width};
    }
    case FAM_A0:
        // linear space: Noll * width + 4 states of 5 ints (H and Noll - 1 vertical-gap states); 4 * Noll link / bound rows per intermediate
        if (T.kind == KIND_UDH) return {5 * (noll * width + 4), 0, n_im * 4 * noll * width};
        // H, F (values, Vmf pointers) and the direction entries by diagonal (+ F2 with Noll = 3); Vmf records
        // (+ what the waves of a pipelined problem may leave unused of the chunks of numbers they reserve)
        return {(noll == 3 ? 7 : 5) * width + 8, T.vmf ? cap + (int64_t) SPDP_VMF_CHUNK * (rows / 64 + 2) : 0, 0};
    default:
        // -A1 and local udh: hv / fv (/ hb / hc / fc) by diagonal, buf ints each, a counter; udh forms: + the `ml` row of F;
        // Noll = 3: + fv2, fc2 behind the counter
        // (Vmf: + what the lanes may leave unused of the chunks of numbers they reserve, per stripe when pipelined)
        return {(T.kind == KIND_UDH ? 6 : (noll == 3 ? 8 : 5)) * buf + 8,
                T.vmf ? cap + (int64_t) 2 * SPDP_VMF_LANE_CHUNK * SPDP_NELEM * (rows / SPDP_NELEM + 2) : 0, n_im * 4 * width};
    }
}

// validates the items and fills h_probs (caller order); tot: the buffers' totals in the units of ItemShare
int DevRun::lay_out(const std::vector<RunItem>& items, ItemShare& tot)
{
    const DevStore* st = store;
    const RunTraits& T = traits();
    h_probs.assign(n, DevProblem());
    tot = {0, 0, 0};
    cut = false; total_cells = 0; max_n_im = 0; max_skl = 0;
    for (int i = 0; i < n; ++i) {
        const RunItem& it = items[i];
        DevProblem& P = h_probs[i];
        if (it.parent < 0 || it.parent >= st->n_parents || it.a_left < 0 || it.b_left < 0 ||
            it.a_right > st->a_len[it.parent] || it.b_right > st->b_len[it.parent] ||
            it.a_right < it.a_left || it.b_right < it.b_left || it.w.width < 3) {
            ctx->err = "bad item ranges"; return -1;
        }
        P.a_left = it.a_left; P.a_right = it.a_right; P.b_left = it.b_left; P.b_right = it.b_right;
        P.lw = it.w.lw; P.up = it.w.up; P.width = it.w.width;
        P.cut_l = P.cut_len = 0;
        if (it.cut_r > it.cut_l) {              // forwardS_ng over a cut range: its arrays are narrower by the cut (src/fwd2s1.cc:234)
            if (flavour != RUN_A0_FORWARD || it.a_exgl || it.w.width - (it.cut_r - it.cut_l) < 3 || it.cut_l < it.b_left ||
                it.cut_r > it.b_right || (i > 0 && !cut)) { ctx->err = "bad cut range"; return -1; }
            cut = true;
            P.cut_l = it.cut_l; P.cut_len = it.cut_r - it.cut_l;
            P.width = it.w.width - P.cut_len;
        } else if (cut) { ctx->err = "bad cut range"; return -1; }
        P.buf_size = it.w.width + 2 * SPDP_NELEM;
        P.flags = (it.a_exgl ? 1 : 0) | (it.a_exgr ? 2 : 0) | (it.b_exgl ? 4 : 0) | (it.b_exgr ? 8 : 0);
        P.n_im = T.rows() ? it.n_im : 0;
        P.imd_intvl = it.imd_intvl;
        P.a_off = st->a_off[it.parent]; P.col_off = st->col_off[it.parent];
        P.cip_off = st->cip_off.empty() ? -1 : st->cip_off[it.parent];
        const ItemShare sh = item_share(T, it, st->sc.noll);
        P.bnd_off = tot.work; P.tb_off = tot.tb;
        P.imd_off = T.vmf ? sh.tb : tot.imd;    // (ScalarArgs::probs: a Vmf-backed problem's record budget goes here)
        tot.work += sh.work; tot.tb += sh.tb; tot.imd += sh.imd;
        P.cells = spdp_cells_w(it.a_left, it.a_right, it.b_left, it.b_right, it.w);
        total_cells += P.cells;
        max_n_im = std::max(max_n_im, P.n_im);
        max_skl = std::max(max_skl, (it.a_right - it.a_left) + (it.b_right - it.b_left) + 8);
    }
    tb_bytes = tot.tb;
    return 0;
}

// fp32 sweeps: every score must stay an exactly representable integer below 2^22 - 2^16 (the penalty table
// pushes a candidate down by 2^22 to disable it).  Upper bound of a score: matches on every row, plus
// whatever an intron can gain where the signals outweigh its penalties (never, with real parameters).
// The step carries the gap opened from a cell unfloored (spdp_sweep_fp.hip, above its STEP): an E or F state at the floor
// must not rise again by extension, so a positive gap extension stays with the int32 sweeps.
static bool fp_range_ok(const DevStore* st, const std::vector<RunItem>& items)
{
    int64_t rows = 0, cols_span = 0;
    for (const RunItem& it : items) {
        rows = std::max<int64_t>(rows, it.a_right - it.a_left);
        cols_span = std::max<int64_t>(cols_span, it.b_right - it.b_left);
    }
    const int64_t ub = (rows + 1) * st->fp_maxpos + (st->fp_gain > 0 ? (cols_span + 1) * st->fp_gain : 0) + 65536;
    return spdp_knob_on("SPDP_FP") && ub < (1ll << 22) - 65536 && st->sc.gep <= 0;
}

int DevRun::allocate(const ItemShare& tot)
{
    const RunTraits& T = traits();
    const int nn = std::max(n, 1);
    skl_cap = std::min(std::max(max_skl, 1), 1024);     // typical lists are short; DevRun::fetch_skl walks the rest again
    if (const char* e = getenv("SPDP_SKL_CAP")) skl_cap = std::max(4, std::min(skl_cap, atoi(e)));   // test hook: tiny slots
    POOLGET(d_probs, POOL_PROBS, sizeof(DevProblem) * nn);
    POOLGET(d_bnd, POOL_BND, sizeof(int32_t) * T.bw * std::max<int64_t>(tot.work, 1));
    POOLGET(d_res, POOL_RES, sizeof(DevResult) * nn);
    if (T.records()) {
        POOLGET(d_tb, POOL_TB, (T.vmf ? sizeof(int3) : 1) * std::max<int64_t>(tot.tb, 16));
        POOLGET(d_skl, POOL_SKL, sizeof(int2) * (int64_t) skl_cap * nn);
        POOLGET(d_nskl, POOL_NSKL, sizeof(int) * nn);
    }
    if (T.rows()) {
        POOLGET(d_imd, POOL_IMD, sizeof(int32_t) * std::max<int64_t>(tot.imd, 1));
        POOLGET(d_cpos, POOL_CPOS, sizeof(int32_t) * cpos_stride() * nn);
        POOLGET(d_ranges, POOL_RANGES, sizeof(int32_t) * 4 * nn);
        POOLGET(d_scores, POOL_SCORES, sizeof(int32_t) * 2 * nn);          // scores, then the left-edge marks of spdp_udh_cpos
    }
    return 0;
}

// dispatch order = largest problems first (longest-processing-time rule): one wave owns one
// problem, so the big ones must not start last.  order[j] = caller index of dispatch slot j.
// Problems that can be spread over a block's waves (>= 16 stripes) come first, see plan_blocks.
void DevRun::sort_dispatch(bool may_multi)
{
    order.resize(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    auto wide = [&](int x) { return may_multi && stripes_of(h_probs[x]) >= 16; };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        const bool wx = wide(x), wy = wide(y);
        return wx != wy ? wx : h_probs[x].cells > h_probs[y].cells;
    });
    std::vector<DevProblem> sorted(n);
    for (int j = 0; j < n; ++j) sorted[j] = h_probs[order[j]];
    h_probs.swap(sorted);
}

// Big problems (>= 16 stripes = 4 passes) are spread over the 4 waves of a block (pipelined passes).
// That pays in full launches too: the longest problem bounds the launch, and the passes of one
// problem running a few blocks apart share their column records in L2.  (Measured on C2, 10000
// queries: 540 -> 652 GCUPS end to end.)  SPDP_MULTI=0 restores one wave per problem.
int DevRun::plan_blocks(bool may_multi)
{
    const SpdpScoring& sc = store->sc;
    n_multi = 0; wpb = 4; cross_g = 0;
    if (!may_multi) return 0;
    if (spdp_knob_on("SPDP_MULTI"))
        while (n_multi < n && stripes_of(h_probs[n_multi]) >= 16) ++n_multi;           // sorted: a prefix
    // a launch of a few huge problems only (top levels of the recursion on a long cDNA): one
    // 16-wave block, i.e. a whole CU, per problem
    if (const char* w16 = getenv("SPDP_WPB16")) { if (atoi(w16) != 0) wpb = 16; }
    else if (n > 0 && n_multi == n && n <= 2 * ctx->n_cu) {
        const int smallest = stripes_of(h_probs[n - 1]);
        if (smallest >= 4 * 32) wpb = 16;                            // >= 32 passes each
        // a handful of mid-sized problems (the stragglers of an EST batch that need the linear-space
        // engine): the launch is latency-bound, more passes in flight shorten it
        else if (!beside && n <= ctx->n_cu / 2 && smallest > 4 * 4) wpb = 16;
    }
    // fewer huge problems than a quarter of the CUs (the top levels of the recursion on one long cDNA): each spread over
    // several CUs -- cross-CU pass pipelines, all blocks resident.  For the linear-space sweep, and for the traceback sweep
    // where spdp_sweep_fp serves it (the tall slabs a long cDNA's recursion leaves, spdp_host.cpp)
    const char* cg = getenv("SPDP_CROSS");
    bool crossable = flavour == RUN_WIP_UDH;
    if (flavour == RUN_WIP_FORWARD && fp_ok && spdp_knob_on("SPDP_FP_FWD")) {
        const int nq = std::max(1, std::min(sc.nquant, SPDP_MAX_QUANT));
        crossable = spdp_sweep_fp_serves(sc.local ? 1 : 0, sc.spj ? 1 : 0, nq, nq > 1 ? sc.qm_len[nq - 2] + 1 : 0, sc.llmt) != 0;
    }
    if (crossable && wpb == 16 && n_multi == n && n > 0 && (!cg || atoi(cg) != 0)) {
        int max_passes = 0, min_passes = 1 << 30;
        for (int j = 0; j < n; ++j) {
            max_passes = std::max(max_passes, (stripes_of(h_probs[j]) + 3) / 4);
            min_passes = std::min(min_passes, (stripes_of(h_probs[j]) + 3) / 4);
        }
        const int room = ctx->n_cu / n;                              // blocks per problem, one block per CU
        int g = std::min(room, (max_passes + 15) / 16);
        // with CUs to spare a wave gets a SIMD to itself: 4-wave blocks, one pass per wave
        const char* c4 = getenv("SPDP_CROSS_WPB");
        if (c4 ? atoi(c4) == 4 : (max_passes + 3) / 4 <= room) { wpb = 4; g = std::min(room, (max_passes + 3) / 4); }
        if (cg && atoi(cg) > 1) g = std::min(room, atoi(cg));
        if (g >= 2 && min_passes >= 32) cross_g = g;
        else wpb = 16;
    }
    if (cross_g > 0) {
        const size_t words = (size_t) n * (cross_g * wpb + 2);
        POOLGET(d_gprog, POOL_GPROG, sizeof(int) * words);
        HIPCHK(hipMemsetAsync(d_gprog, 0, sizeof(int) * words, strm()));
    }
    return 0;
}

// a problem's tiles / stripes as a pipeline of waves (TilePipe; SPDP_A1_PIPE=0, SPDP_A0_PIPE=0: one wave each)
int DevRun::plan_pipe()
{
    const RunTraits& T = traits();
    pipe = TilePipe();
    if (!T.pipe_tpw || n == 0) return 0;
    if (T.family == FAM_A1) pipe.plan_groups(h_probs, 4);   // work item = (four problems, 16-row stripe), spdp_exact<., true>
    else                                                    // forwardS_ng / scorealoneS_ng: 64-row tiles; hirschbergS_ng: imd_intvl rows
        for (int j = 0; j < n; ++j) {
            const DevProblem& P = h_probs[j];
            pipe.plan(j, P.a_right - (P.a_left + (P.flags & 1)), T.kind == KIND_UDH ? std::max(1, std::min(64, P.imd_intvl)) : 64);
        }
    const bool wanted = spdp_knob_on(T.family == FAM_A1 ? "SPDP_A1_PIPE" : "SPDP_A0_PIPE") && pipe.max_tiles >= 2 && !cut;
    if (wanted && !pipe.reserve(pool(), POOL_GPROG, n, T.pipe_tpw, max_n_im)) { ctx->err = "out of device memory"; return -1; }
    return 0;
}

int DevRun::build(const DevStore* st, const std::vector<RunItem>& items, RunFlavour flav)
{
    store = st; ctx = use_ctx ? use_ctx : st->ctx; flavour = flav; n = (int) items.size();
    (void) hipSetDevice(ctx->device);
    if (check()) return -1;
    // hirschbergS1_wip with local ends (-LS): its own kernel (spdp_local_udh.hip)
    if (flavour == RUN_WIP_UDH && st->sc.local) flavour = RUN_LOCAL_UDH;
    const bool may_multi = traits().family == FAM_WIP && !st->sc.local;     // problems spread over the waves of a block
    ItemShare tot;
    if (lay_out(items, tot)) return -1;
    fp_ok = fp_range_ok(st, items);
    if (allocate(tot)) return -1;
    sort_dispatch(may_multi);
    if (plan_blocks(may_multi) || plan_pipe()) return -1;
    if (n) HIPCHK(hipMemcpyAsync(d_probs, h_probs.data(), sizeof(DevProblem) * n, hipMemcpyHostToDevice, strm()));
    return 0;
}

// the link walk (spdp_udh_cpos) behind a linear-space sweep; pipe_words: the sync words of a pipelined spdp_exact<2>, or null
CposArgs DevRun::cpos_args(int strict, int local, const int* pipe_words) const
{
    CposArgs C{};
    C.probs = (const DevProblem*) d_probs; C.n_probs = n; C.imd = (const int*) d_imd; C.res = (const DevResult*) d_res;
    C.cpos = (int*) d_cpos; C.ranges = (int*) d_ranges; C.scores = (int*) d_scores;
    C.cpos_stride = cpos_stride(); C.strict = strict; C.local = local;
    C.edge = (int*) d_scores + n;
    C.pipe = pipe_words; C.pipe_stride = pipe.stride; C.rlf_off = pipe.rlf_off;
    return C;
}

int DevRun::launch()
{
    const RunTraits& T = traits();
    (void) hipSetDevice(ctx->device);
    if (n == 0) return 0;
    in_flight = true;
    if (T.launcher == BY_SWEEP ? launch_sweep() : launch_scalar()) return -1;
    if (T.edge) {                           // hirschbergS1_wip's / hirschbergS1's / the local hirschbergS1_wip's link walk
        const bool a1 = T.family == FAM_A1;
        const CposArgs C = cpos_args(a1, store->sc.local ? 1 : 0, a1 && pipe.on ? pipe.d : nullptr);
        HIPCHK(spdp_launch_cpos(&C, strm()));
    }
    return 0;
}

// the -A0, -A1 and local engines
int DevRun::launch_scalar()
{
    const RunTraits& T = traits();
    ScalarArgs S{};
    HIPCHK(pipe.arm(strm(), n, S));
    S.sc = (const DevScoring*) store->d_sc; S.probs = (const DevProblem*) d_probs; S.n_probs = n;
    S.a_codes = (const uint8_t*) store->d_a; S.cols = (const int2*) store->d_cols;
    S.aux = (const uint8_t*) store->d_aux; S.intpen = (const int16_t*) store->d_intpen;
    S.ipen_runs = (const int16_t*) store->d_ipen_runs; S.cip = (const int*) store->d_cip;
    S.intpen_len = store->sc.intpen_len; S.ipen = store->sc.ipen;
    memcpy(S.t53, store->sc.t53, sizeof S.t53);
    S.work = (int*) d_bnd; S.vmf = (int3*) d_tb; S.res = (DevResult*) d_res;
    S.skl = (int2*) d_skl; S.n_skl = (int*) d_nskl; S.skl_cap = skl_cap;
    S.imd = (int*) d_imd; S.cpos = (int*) d_cpos; S.ranges = (int*) d_ranges; S.scores = (int*) d_scores;
    S.cpos_stride = cpos_stride();
    HIPCHK(hipEventRecord(evb(), strm()));
    S.minl = store->sc.minl ? store->sc.minl : store->sc.llmt;
    S.noll = store->sc.noll; S.lgop = store->sc.lgop; S.lgep = store->sc.lgep; S.codonk1 = store->sc.codonk1;
    switch (T.launcher) {
    case BY_LOCAL_UDH:   HIPCHK(spdp_launch_local_udh(&S, strm())); break;
    case BY_EXACT:       HIPCHK(spdp_launch_exact(T.arg, &S, strm())); break;
    case BY_ROWWAVE_UDH: HIPCHK(spdp_launch_rowwave_udh(&S, strm())); break;
    default:             HIPCHK(spdp_launch_rowwave(cut ? 2 : T.arg, &S, strm())); break;    // (cut: RUN_A0_FORWARD only, lay_out)
    }
    HIPCHK(hipEventRecord(eve(), strm()));
    return 0;
}

// the `_wip` sweeps
int DevRun::launch_sweep()
{
    const RunTraits& T = traits();
    SweepArgs A;
    A.sc = (const DevScoring*) store->d_sc; A.probs = (const DevProblem*) d_probs; A.n_probs = n;
    A.a_codes = (const uint8_t*) store->d_a; A.cols = (const int2*) store->d_cols; A.bnd = (int*) d_bnd;
    A.tb = (uint8_t*) d_tb; A.imd = (int*) d_imd; A.res = (DevResult*) d_res; A.n_multi = n_multi;
    A.cross_g = cross_g; A.gprog = (int*) d_gprog;
    // the start signal rides on the plain 4-wave launch of the linear-space sweep only (cooperative and 16-wave launches,
    // and every other flavour, leave the pointers null: those kernels do not look at them)
    A.started = nullptr; A.started_host = nullptr;
    signal_armed = signal_start && flavour == RUN_WIP_UDH && cross_g == 0 && wpb == 4 && !store->sc.local;
    if (signal_armed) {
        if (ctx->start_signal()) return -1;
        HIPCHK(hipMemsetAsync(ctx->d_started, 0, sizeof(unsigned), strm()));
        __atomic_store_n(ctx->sig_host, 0, __ATOMIC_RELEASE);
        A.started = ctx->d_started; A.started_host = ctx->sig_host_dev;
    }
    int grid = cross_g > 0 ? n * cross_g : n_multi + (n - n_multi + wpb - 1) / wpb;
    if (cross_g > 0 && getenv("SPDP_CROSS_TEST_SHORT")) --grid;    // test hook: one block never arrives -> the fallback runs
    HIPCHK(hipEventRecord(evb(), strm()));
    const int nq = std::max(1, std::min(store->sc.nquant, SPDP_MAX_QUANT));
    const int pen_cap = nq > 1 ? store->sc.qm_len[nq - 2] + 1 : 0;
    // the fp32-issue form of the sweep (spdp_sweep_fp.hip) where it applies: non-local runs whose scores stay inside the
    // exact fp32 integer range; SPDP_FP=0 keeps everything on spdp_kernels.hip, SPDP_FP_FWD=0 the traceback sweep
    bool done = false;
    if (fp_ok && (T.kind != KIND_FORWARD || spdp_knob_on("SPDP_FP_FWD")) && !store->sc.local) {
        const hipError_t e = spdp_launch_sweep_fp(T.arg, 0, store->sc.spj ? 1 : 0, nq, pen_cap, store->sc.llmt, &A, grid, wpb, strm());
        if (e == hipSuccess) done = true;
        else if (e != hipErrorNotSupported) HIPCHK(e);
    }
    if (!done) HIPCHK(spdp_launch_sweep(T.arg, store->sc.local ? 1 : 0, nq, pen_cap, &A, grid, wpb, strm()));
    ++ctx->sweep_stats[done ? 0 : 1];
    if (cross_g > 0) ++ctx->sweep_stats[2];
    if (wpb == 16) ++ctx->sweep_stats[3];
    HIPCHK(hipEventRecord(eve(), strm()));
    if (T.records()) {
        WalkArgs W;
        W.probs = A.probs; W.n_probs = n; W.tb = (const uint8_t*) d_tb; W.res = (const DevResult*) d_res;
        W.skl = (int2*) d_skl; W.n_skl = (int*) d_nskl; W.skl_cap = skl_cap;
        { const char* sw = getenv("SPDP_WALK_SEQ"); W.seq = (sw && atoi(sw) != 0) ? 1 : 0; }
        HIPCHK(spdp_launch_walk(&W, strm()));
    }
    return 0;
}

extern "C" void spdp_rerun_stats(SpdpContext* ctx, int64_t* out, int reset)
{
    if (!ctx || !out) return;
    out[0] = ctx->rerun_stats[0]; out[1] = ctx->rerun_stats[1];
    if (reset) ctx->rerun_stats[0] = ctx->rerun_stats[1] = 0;
    for (SpdpContext* l : ctx->lanes) {                     // chunks of a batch run on the context's lanes
        out[0] += l->rerun_stats[0]; out[1] += l->rerun_stats[1];
        if (reset) l->rerun_stats[0] = l->rerun_stats[1] = 0;
    }
}

extern "C" void spdp_sweep_stats(SpdpContext* ctx, int64_t* out, int reset)
{
    if (!ctx || !out) return;
    for (int k = 0; k < 4; ++k) {
        out[k] = reset ? ctx->sweep_stats[k].exchange(0) : ctx->sweep_stats[k].load();
        for (SpdpContext* l : ctx->lanes)                   // chunks of a batch run on the context's lanes
            out[k] += reset ? l->sweep_stats[k].exchange(0) : l->sweep_stats[k].load();
    }
}

extern "C" void spdp_chunk_stats(SpdpContext* ctx, int64_t* out, int reset)
{
    if (!ctx || !out) return;
    for (int k = 0; k < 6; ++k) out[k] = reset ? ctx->chunk_stats[k].exchange(0) : ctx->chunk_stats[k].load();
}

int DevRun::sync()
{
    HIPCHK(hipStreamSynchronize(strm()));
    in_flight = false;
    if (cross_g > 0) {
        // cross-CU pipelines need every block resident; on a shared GPU the start-up barrier can time out, the
        // blocks then leave a mark (second barrier word of their problem) and the launch is repeated without them
        const size_t per = (size_t) cross_g * wpb + 2;
        std::vector<int> words(per * n);
        HIPCHK(spdp_copy_sync(words.data(), d_gprog, sizeof(int) * words.size(), hipMemcpyDeviceToHost, strm()));
        bool gave_up = false;
        for (int j = 0; j < n; ++j) gave_up = gave_up || words[per * j + per - 1] != 0;
        if (gave_up) {
            ++ctx->rerun_stats[0];
            if (getenv("SPDP_TRACE_RUNS")) fprintf(stderr, "[spdp run] a cross-CU group was not resident%s: launch repeated without the groups\n", side ? " (side stream, beside another launch)" : "");
            cross_g = 0; wpb = 16;
            if (launch()) return -1;
            HIPCHK(hipStreamSynchronize(strm()));
        }
    }
    bool gave_up = false;                               // a wave waited in vain for the tile above it: repeated with one wave per problem
    HIPCHK(pipe.stalled(strm(), n, &gave_up));
    if (gave_up) {
        ++ctx->rerun_stats[1];
        pipe.on = false;
        if (launch()) return -1;
        HIPCHK(hipStreamSynchronize(strm()));
    }
    kernel_ms = 0.f;
    if (n) HIPCHK(hipEventElapsedTime(&kernel_ms, evb(), eve()));
    if (n && getenv("SPDP_TRACE_RUNS")) {
        int mr = 0, mc = 0; int64_t mcell = 0;
        for (int j = 0; j < n; ++j) {
            mr = std::max(mr, h_probs[j].a_right - h_probs[j].a_left); mc = std::max(mc, h_probs[j].width);
            mcell = std::max<int64_t>(mcell, h_probs[j].cells);
        }
        fprintf(stderr, "[spdp run] flavour %d n %d cells %.3g (largest %.3g, rows <= %d, width <= %d) pipe %d items %zu  %.2f ms  %.1f GCUPS\n",
                (int) flavour, n, (double) total_cells, (double) mcell, mr, mc, (int) pipe.on, pipe.items.size() / 2, kernel_ms,
                total_cells / (kernel_ms * 1e6));
    }
    return 0;
}

int DevRun::fetch_results(std::vector<DevResult>& out)
{
    out.resize(n);
    std::vector<DevResult> tmp(n);
    if (n) HIPCHK(spdp_copy_sync(tmp.data(), d_res, sizeof(DevResult) * n, hipMemcpyDeviceToHost, strm()));
    for (int j = 0; j < n; ++j) out[order[j]] = tmp[j];
    return 0;
}

int DevRun::fetch_skl(std::vector<int>& n_skl, std::vector<int64_t>& off, std::vector<SpdpSkl>& skl)
{
    n_skl.assign(n, 0); off.assign(n + 1, 0);
    if (!n) { skl.clear(); return 0; }
    std::vector<int> cnt(n);                            // dispatch order
    HIPCHK(spdp_copy_sync(cnt.data(), d_nskl, sizeof(int) * n, hipMemcpyDeviceToHost, strm()));
    // Lists that did not fit their slot (skl_cap is sized for typical lists; an indel-rich slab can need more): the
    // walk is repeated for those few with slots of the longest list their problem can produce.  Only the `_wip`
    // walk (RUN_WIP_FORWARD) can be repeated on its own; the scalar / -A1 engines walk inside their sweep kernel and
    // report the overflow (-1) to the caller, who gives up that one query, not the batch.
    std::vector<int> over;
    for (int j = 0; j < n; ++j) if (cnt[j] == -1) over.push_back(j);
    std::vector<std::vector<SpdpSkl>> redo(over.size());
    if (!over.empty() && flavour == RUN_WIP_FORWARD) {
        const int m = (int) over.size();
        std::vector<DevResult> all_res(n), sub_res(m);
        std::vector<DevProblem> sub_probs(m);
        HIPCHK(spdp_copy_sync(all_res.data(), d_res, sizeof(DevResult) * n, hipMemcpyDeviceToHost, strm()));
        int cap2 = 1;
        for (int k = 0; k < m; ++k) {
            const DevProblem& P = h_probs[over[k]];
            sub_probs[k] = P; sub_res[k] = all_res[over[k]];
            cap2 = std::max(cap2, (P.a_right - P.a_left) + (P.b_right - P.b_left) + 8);
        }
        void *dp = nullptr, *dr = nullptr, *ds = nullptr, *dn = nullptr;
        HIPCHK(hipMalloc(&dp, sizeof(DevProblem) * m));
        HIPCHK(hipMalloc(&dr, sizeof(DevResult) * m));
        HIPCHK(hipMalloc(&ds, sizeof(int2) * (size_t) cap2 * m));
        HIPCHK(hipMalloc(&dn, sizeof(int) * m));
        HIPCHK(spdp_copy_sync(dp, sub_probs.data(), sizeof(DevProblem) * m, hipMemcpyHostToDevice, strm()));
        HIPCHK(spdp_copy_sync(dr, sub_res.data(), sizeof(DevResult) * m, hipMemcpyHostToDevice, strm()));
        WalkArgs W;
        W.probs = (const DevProblem*) dp; W.n_probs = m; W.tb = (const uint8_t*) d_tb; W.res = (const DevResult*) dr;
        W.skl = (int2*) ds; W.n_skl = (int*) dn; W.skl_cap = cap2; W.seq = 0;
        HIPCHK(spdp_launch_walk(&W, strm()));
        HIPCHK(hipStreamSynchronize(strm()));
        std::vector<int> c2(m);
        HIPCHK(spdp_copy_sync(c2.data(), dn, sizeof(int) * m, hipMemcpyDeviceToHost, strm()));
        for (int k = 0; k < m; ++k) {
            cnt[over[k]] = c2[k];
            if (c2[k] > 0) {
                redo[k].resize(c2[k]);
                HIPCHK(spdp_copy_sync(redo[k].data(), (const int2*) ds + (size_t) k * cap2, sizeof(SpdpSkl) * c2[k], hipMemcpyDeviceToHost, strm()));
            }
        }
        (void) hipFree(dp); (void) hipFree(dr); (void) hipFree(ds); (void) hipFree(dn);
    }
    std::vector<int64_t> doff(n + 1, 0);
    for (int j = 0; j < n; ++j) {
        if (cnt[j] > skl_cap && redo.empty()) { ctx->err = "traceback record list exceeds the per-problem slot"; return -1; }
        // (cnt = -3: the call outgrew its Vmf record budget; the ladder runs it again with a larger one)
        doff[j + 1] = doff[j] + std::max(cnt[j], 0);
        n_skl[order[j]] = cnt[j];
    }
    std::vector<SpdpSkl> packed(doff[n]);
    if (doff[n]) {
        void *d_off, *d_pack;
        POOLGET(d_off, POOL_SKLOFF, sizeof(int64_t) * (n + 1));
        POOLGET(d_pack, POOL_SKLPACK, sizeof(int2) * doff[n]);
        HIPCHK(hipMemcpyAsync(d_off, doff.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, strm()));
        HIPCHK(spdp_launch_pack((const int2*) d_skl, skl_cap, (const int*) d_nskl, (const int64_t*) d_off,
                                (int2*) d_pack, n, strm()));
        HIPCHK(hipMemcpyAsync(packed.data(), d_pack, sizeof(SpdpSkl) * doff[n], hipMemcpyDeviceToHost, strm()));
        HIPCHK(hipStreamSynchronize(strm()));
    }
    // back to the caller's order
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + std::max(n_skl[i], 0);
    skl.resize(off[n]);
    for (int j = 0; j < n; ++j)
        if (cnt[j] > 0) memcpy(skl.data() + off[order[j]], packed.data() + doff[j], sizeof(SpdpSkl) * cnt[j]);
    for (size_t k = 0; k < over.size(); ++k)            // the lists of the second walk (the pack kernel skipped them)
        if (!redo[k].empty()) memcpy(skl.data() + off[order[over[k]]], redo[k].data(), sizeof(SpdpSkl) * redo[k].size());
    return 0;
}

int DevRun::fetch_udh(std::vector<int32_t>& scores, std::vector<int32_t>& cpos, std::vector<int32_t>& ranges,
                      std::vector<int32_t>* edge)
{
    const size_t st = cpos_stride();
    scores.resize(n); ranges.resize((size_t) 4 * n); cpos.resize(st * n);
    if (edge) edge->assign(n, 0);
    if (n) {
        std::vector<int32_t> ts(n), tr((size_t) 4 * n), tc(st * n);
        HIPCHK(spdp_copy_sync(ts.data(), d_scores, sizeof(int32_t) * n, hipMemcpyDeviceToHost, strm()));
        if (edge && traits().edge) {
            std::vector<int32_t> te(n);
            HIPCHK(spdp_copy_sync(te.data(), (int32_t*) d_scores + n, sizeof(int32_t) * n, hipMemcpyDeviceToHost, strm()));
            for (int j = 0; j < n; ++j) (*edge)[order[j]] = te[j];
        }
        HIPCHK(spdp_copy_sync(tr.data(), d_ranges, sizeof(int32_t) * 4 * n, hipMemcpyDeviceToHost, strm()));
        HIPCHK(spdp_copy_sync(tc.data(), d_cpos, sizeof(int32_t) * tc.size(), hipMemcpyDeviceToHost, strm()));
        for (int j = 0; j < n; ++j) {
            const int i = order[j];
            scores[i] = ts[j];
            memcpy(&ranges[(size_t) 4 * i], &tr[(size_t) 4 * j], sizeof(int32_t) * 4);
            memcpy(&cpos[st * i], &tc[st * j], sizeof(int32_t) * st);
        }
    }
    return 0;
}

// ---- engine-level entry points (SimdAln2s1 methods) -----------------------------------------
static std::vector<RunItem> items_of(const SpdpScoring* sc, const SpdpProblem* probs, int n)
{
    std::vector<RunItem> v(n);
    for (int i = 0; i < n; ++i) v[i] = spdp_item_of(probs[i], i, sc->sh);
    return v;
}

static int score_like(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs, int n_probs, int32_t* scores, RunFlavour flav)
{
    if (!ctx) return -1;
    if (n_probs <= 0) return 0;
    DevStore st; DevRun run;
    std::vector<DevResult> r;
    if (st.upload(ctx, sc, probs, n_probs)) return -1;
    if (run.build(&st, items_of(sc, probs, n_probs), flav) || run.launch() || run.sync() || run.fetch_results(r)) return -1;
    for (int i = 0; i < n_probs; ++i) scores[i] = r[i].score;
    return 0;
}

int spdp_wip_scoreonly(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs, int n_probs, int32_t* scores)
{
    return score_like(ctx, sc, probs, n_probs, scores, RUN_WIP_SCORE);
}

// HomScoreS_ng on an uploaded store (src/fwd2s1.cc:2696-2716): scoreonlyS1_wip on the stripe() band for
// simd > 1; scorealoneS_ng when simd == 0 or the query range has fewer than 4 rows.  Returns 1 when a
// problem needs the scalar engine and its inputs are missing (score NEVSEL).
static int homscore_on_store(SpdpContext* ctx, const DevStore& st, const SpdpProblem* probs, int n_probs, int32_t* scores)
{
    const SpdpScoring* sc = &st.sc;
    const RunFlavour leg_flav[3] = {RUN_WIP_SCORE, RUN_A0_SCORE, RUN_A1_SCORE};     // -A1: scoreonlyS1
    std::vector<RunItem> items[3];
    std::vector<int> at[3];
    int rc = 0;
    for (int i = 0; i < n_probs; ++i) {
        scores[i] = SPDP_NEVSEL;
        const RunItem it = spdp_item_of(probs[i], i, sc->sh);
        const int leg = (sc->scalar_engines == 1 || it.a_right - it.a_left < 4) ? 1 : (sc->scalar_engines == 2 ? 2 : 0);
        if (it.w.width < 3 || (leg && !st.has_exact)) { rc = 1; continue; }
        items[leg].push_back(it); at[leg].push_back(i);
    }
    for (int leg = 0; leg < 3; ++leg) {
        DevRun run;
        std::vector<DevResult> r;
        if (items[leg].empty()) continue;
        if (run.build(&st, items[leg], leg_flav[leg]) || run.launch() || run.sync() || run.fetch_results(r)) return -1;
        for (size_t k = 0; k < r.size(); ++k) scores[at[leg][k]] = r[k].score;
    }
    return rc;
}

int spdp_homscore_s(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs,
                    int n_probs, int32_t* scores)
{
    if (!ctx || !sc || !probs || !scores) return -1;
    if (n_probs <= 0) return 0;
    DevStore st;
    if (st.upload(ctx, sc, probs, n_probs)) return -1;
    return homscore_on_store(ctx, st, probs, n_probs, scores);
}

// a linear-space engine on whole problems: n_im intermediate rows each, imd_intvl apart (-A0; 0: the engine's own spacing);
// flags: DevResult::pad[0] per problem, or null
static int udh_like(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs, int n_probs, RunFlavour flav, int n_im,
                    int imd_intvl, int32_t* scores, int32_t* cpos, int32_t* ranges, int32_t* flags)
{
    if (n_probs <= 0) return 0;
    DevStore st; DevRun run;
    if (st.upload(ctx, sc, probs, n_probs)) return -1;
    std::vector<RunItem> items = items_of(sc, probs, n_probs);
    for (auto& it : items) {
        it.n_im = n_im; it.imd_intvl = imd_intvl;
        if (imd_intvl > 0 && it.a_left + (int64_t) n_im * imd_intvl > it.a_right + imd_intvl) { ctx->err = "intermediate rows beyond the query range"; return -1; }
    }
    if (run.build(&st, items, flav) || run.launch() || run.sync()) return -1;
    std::vector<int32_t> s, c, r;
    std::vector<DevResult> res;
    if (run.fetch_udh(s, c, r) || (flags && run.fetch_results(res))) return -1;
    memcpy(scores, s.data(), sizeof(int32_t) * n_probs);
    memcpy(ranges, r.data(), sizeof(int32_t) * 4 * n_probs);
    memcpy(cpos, c.data(), sizeof(int32_t) * c.size());
    for (int i = 0; flags && i < n_probs; ++i) flags[i] = res[i].pad[0];
    return 0;
}

int spdp_wip_udh(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs, int n_probs,
                 int n_im, int32_t* scores, int32_t* cpos, int32_t* ranges)
{
    return ctx ? udh_like(ctx, sc, probs, n_probs, RUN_WIP_UDH, n_im, 0, scores, cpos, ranges, nullptr) : -1;
}

int spdp_scalar_udh(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs, int n_probs,
                    int n_im, int imd_intvl, int32_t* scores, int32_t* cpos, int32_t* ranges, int32_t* flags)
{
    if (!ctx || !sc || !probs || !scores || !cpos || !ranges || !flags || n_im < 1 || imd_intvl < 1) return -1;
    // test hook: the same call on hirschbergS1 (the -A1 linear-space engine, spdp_exact<2> + spdp_udh_cpos), which the ABI
    // otherwise reaches through alignS_ng only; imd_intvl is then the engine's own (a_right - a_left + n_im) / (n_im + 1)
    const RunFlavour flav = getenv("SPDP_UDH_ENGINE_A1") ? RUN_A1_UDH : RUN_A0_UDH;
    return udh_like(ctx, sc, probs, n_probs, flav, n_im, imd_intvl, scores, cpos, ranges, flags);
}

static int forward_like(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs, int n_probs,
                        SpdpAlignment* out, RunFlavour flav)
{
    if (!ctx) return -1;
    for (int i = 0; i < n_probs; ++i) { out[i].score = SPDP_NEVSEL; out[i].n_skl = 0; out[i].skl = nullptr; out[i].flags = 0; out[i].reserved = 0; }
    if (n_probs <= 0) return 0;
    DevStore st; DevRun run;
    if (st.upload(ctx, sc, probs, n_probs)) return -1;
    std::vector<RunItem> items = items_of(sc, probs, n_probs);
    for (RunItem& it : items) it.vmf_scale = 1 << 20;           // engine-level call: the full record budget at once
    if (run.build(&st, items, flav) || run.launch() || run.sync()) return -1;
    std::vector<DevResult> r;
    std::vector<int> nskl;
    std::vector<int64_t> off;
    std::vector<SpdpSkl> skl;
    if (run.fetch_results(r) || run.fetch_skl(nskl, off, skl)) return -1;
    for (int i = 0; i < n_probs; ++i) {
        out[i].score = r[i].score;
        if (nskl[i] < 0) { ctx->err = "traceback failed"; return -1; }
        out[i].n_skl = nskl[i];
        out[i].skl = (SpdpSkl*) malloc(sizeof(SpdpSkl) * std::max(1, nskl[i]));
        memcpy(out[i].skl, skl.data() + off[i], sizeof(SpdpSkl) * nskl[i]);
    }
    return 0;
}

int spdp_scalar_forward(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs,
                        int n_probs, SpdpAlignment* out)
{   // Aln2s1::forwardS_ng through trcbkalignS_ng (scalar exact engine)
    return forward_like(ctx, sc, probs, n_probs, out, RUN_A0_FORWARD);
}

int spdp_scalar_scorealone(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs, int n_probs, int32_t* scores)
{   // Aln2s1::scorealoneS_ng = HomScoreS_ng under -A0
    return score_like(ctx, sc, probs, n_probs, scores, RUN_A0_SCORE);
}

int spdp_wip_forward(SpdpContext* ctx, const SpdpScoring* sc, const SpdpProblem* probs,
                     int n_probs, SpdpAlignment* out)
{
    return forward_like(ctx, sc, probs, n_probs, out, RUN_WIP_FORWARD);
}

void spdp_free_alignments(SpdpAlignment* out, int n)
{
    for (int i = 0; i < n; ++i) { free(out[i].skl); out[i].skl = nullptr; out[i].flags = 0; out[i].reserved = 0; out[i].n_skl = 0; }
}
