// lumahip_host.hip -- the _host entry points of include/lumahip.h: staging buffers, host <-> device transfers, and the one
// 3-stage pipeline (upload | kernel | download) behind the banded, batched and stream push / pop forms.  No kernels here.
#include "lumahip_internal.hpp"
#include "half_stage.hpp"

#include <atomic>
#include <condition_variable>
#include <thread>

using namespace lh;
using namespace lhost;

// The fused kernels run on the stream an entry point of this file names in its launch options -- the context's stream, or the
// kernel stream of its pipeline -- and never on a lane of an open unordered section: the uploads and downloads around them are
// ordered against that stream's events (include/lumahip.h: only the four _device encode / decode entry points take part in a
// section).  Frames in the staging buffers are packed, one per launch, their code planes back to back (no frame stride).
static const size_t NO_PFS[3] = {0, 0, 0};

// ---- host <-> device transfers of the _host entry points --------------------------------------------------------
// Caller memory is pageable unless the caller pinned it (hipHostMalloc, hipHostRegister / lumahip_host_register).
// Pinned memory is handed to the copy engine directly (asynchronous, the fast path of the batched entry points).
// Pageable memory is NOT handed to hipMemcpy*Async: the runtime then pins the caller's pages on the fly and caches
// that pinning, and on this stack (ROCm 7.2, MI355X) the GPU occasionally faulted on such a range when host buffers are
// allocated and freed at a high rate ("Memory access fault by GPU ... on address <host heap page>", about one run of
// the GPU test suite in twenty).  Pageable data therefore moves through a ring of context-owned pinned chunks per direction:
// the CPU fills (empties) one chunk while the DMAs of the previous ones are in flight.
static constexpr size_t XFER_CHUNK = (size_t)8 << 20;

// ---- copy threads ---------------------------------------------------------------------------------------------------------
// One CPU thread copies pageable memory into a pinned chunk at ~21 GB/s on the GPU box's host, a third of what the PCIe
// link moves (profiles/r02_hostfed.txt: 1.4 Gpixel/s pageable against 4.2 pinned).  The staging copies are therefore split
// over a few persistent worker threads owned by the context (lumahip_tune "copy_threads", default 5; 0 = the calling thread
// alone): the CPU side then keeps up with the DMA of the previous chunk.
struct lumahip_copy_pool {
    struct Job {
        unsigned char *dst;
        const unsigned char *src;
        size_t width, rows, dst_pitch, src_pitch;  // rows x width bytes; rows == 1: one flat span
        bool to_half = false;                      // flat span of `width` bytes of floats -> width / 2 bytes of halves (half_stage.cpp)
    };
    std::atomic<bool> inexact{false};   // a to_half job met a value that is not a half (raised by any worker, read by copy_to_half)
    // A worker that has just finished a piece polls for the next one for ~0.5 ms before it goes to sleep on the condition
    // variable: while a frame streams through, the pieces follow each other within tens of microseconds, and waking a
    // sleeping thread costs 50-100 us on the GPU box's host -- as much as copying the piece (a 4K band is 8 MB).
    int spin = 2000;
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_go;
    std::vector<Job> jobs;     // one per worker for the current generation
    std::atomic<unsigned> generation{0};
    std::atomic<int> pending{0};
    std::atomic<bool> stop{false};

    // cpus: the CPUs of the GPU's NUMA node the workers are pinned to (empty, the default: wherever the scheduler puts them;
    // lumahip_tune "numa" 1) -- they write the pinned staging chunks, which live on that node, and read them back out of it
    lumahip_copy_pool(int n, int spin_, const std::vector<int> &cpus) : spin(spin_)   // (spin is set before the workers exist: they read it without synchronisation)
    {
        jobs.resize(n);
        for (int i = 0; i < n; i++) {
            workers.emplace_back([this, i]() { loop(i); });
            if (!cpus.empty())
                (void)lh::numa_pin_thread(workers.back().native_handle(), cpus);
        }
    }
    ~lumahip_copy_pool()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop.store(true);
        }
        cv_go.notify_all();
        for (auto &t : workers)
            t.join();
    }
    void run_job(const Job &j)
    {
        if (j.to_half) {
            if (!lh::convert_f32_to_f16_checked(static_cast<const float *>(static_cast<const void *>(j.src)), static_cast<uint16_t *>(static_cast<void *>(j.dst)), j.width / 4))
                inexact.store(true, std::memory_order_relaxed);
            return;
        }
        run(j);
    }
    static void run(const Job &j)
    {
        if (j.rows == 1) {
            memcpy(j.dst, j.src, j.width);
        } else {
            for (size_t r = 0; r < j.rows; r++)
                memcpy(j.dst + r * j.dst_pitch, j.src + r * j.src_pitch, j.width);
        }
    }
    void loop(int me)
    {
        unsigned seen = 0;
        for (;;) {
            int spins = 0;
            unsigned g;
            while ((g = generation.load(std::memory_order_acquire)) == seen) {
                if (stop.load(std::memory_order_relaxed))
                    return;
                if (++spins < spin) {
                    __builtin_ia32_pause();
                    continue;
                }
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&] { return stop.load() || generation.load() != seen; });
            }
            seen = g;
            const Job j = jobs[me];
            if (j.width)
                run_job(j);
            pending.fetch_sub(1, std::memory_order_release);
        }
    }
    // One generation of work: part(k + 1) goes to worker k, part(0) is done here, and the call returns when every part is done
    // (a part of width 0 is nothing to do).  The jobs are published by the generation bump; the lock around it is what a
    // worker about to sleep re-checks the generation under.
    template <typename Part>
    __attribute__((visibility("hidden"))) void dispatch(Part part)
    {
        for (size_t k = 0; k < workers.size(); k++)
            jobs[k] = part(k + 1);
        pending.store((int)workers.size(), std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> lk(mu);
            generation.fetch_add(1, std::memory_order_release);
        }
        cv_go.notify_all();
        const Job mine = part(0);
        if (mine.width)
            run_job(mine);
        while (pending.load(std::memory_order_acquire) != 0)
            __builtin_ia32_pause();
    }
    // rows x width bytes from src (pitch sp) to dst (pitch dp), split over the workers and the calling thread
    void copy(unsigned char *dst, size_t dp, const unsigned char *src, size_t sp, size_t width, size_t rows)
    {
        const size_t parts = workers.size() + 1;
        const bool flat = rows == 1;
        const size_t total = flat ? width : rows;
        if (total * (flat ? 1 : width) < ((size_t)256 << 10) || total < parts) {  // small: not worth handing out
            run(Job{dst, src, width, rows, dp, sp});
            return;
        }
        // flat spans are cut at 4 KiB boundaries so that no two threads share a page
        size_t per = (total + parts - 1) / parts;
        if (flat)
            per = (per + 4095) & ~(size_t)4095;
        dispatch([&](size_t k) -> Job {
            const size_t a = std::min(total, k * per), b = std::min(total, (k + 1) * per);
            if (a >= b)
                return Job{nullptr, nullptr, 0, 0, 0, 0};
            return flat ? Job{dst + a, src + a, b - a, 1, 0, 0} : Job{dst + a * dp, src + a * sp, width, b - a, dp, sp};
        });
    }
    // n floats at src -> n halves at dst, split over the workers and the calling thread (spans cut at multiples of 2048 floats);
    // false when some value is not a half (dst is then useless)
    bool copy_to_half(uint16_t *dst, const float *src, size_t n)
    {
        inexact.store(false, std::memory_order_relaxed);
        const size_t parts = workers.size() + 1;
        if (n < ((size_t)64 << 10) || n < parts)
            return lh::convert_f32_to_f16_checked(src, dst, n);
        const size_t per = ((n + parts - 1) / parts + 2047) & ~(size_t)2047;
        dispatch([&](size_t k) -> Job {
            const size_t a = std::min(n, k * per), b = std::min(n, (k + 1) * per);
            if (a >= b)
                return Job{nullptr, nullptr, 0, 0, 0, 0};
            return Job{reinterpret_cast<unsigned char *>(dst + a), reinterpret_cast<const unsigned char *>(src + a), (b - a) * 4, 1, 0, 0, true};
        });
        return !inexact.load(std::memory_order_relaxed);
    }
};

void lumahip_copy_pool_destroy(lumahip_copy_pool *p) { delete p; }

// the context's copy threads, started on first use; nullptr: none ("copy_threads" 0), the calling thread copies alone
static lumahip_copy_pool *copy_pool(lumahip_ctx *c)
{
    if (c->copy_threads > 0 && !c->copy_pool) {
        numa_resolve(c);
        c->copy_pool = new lumahip_copy_pool(c->copy_threads, c->copy_spin, c->numa_mode == 2 ? std::vector<int>() : c->numa_cpus);
    }
    return c->copy_pool;
}

static void staged_copy(lumahip_ctx *c, unsigned char *dst, size_t dp, const unsigned char *src, size_t sp, size_t width, size_t rows)
{
    if (lumahip_copy_pool *pool = copy_pool(c))
        pool->copy(dst, dp, src, sp, width, rows);
    else
        lumahip_copy_pool::run(lumahip_copy_pool::Job{dst, src, width, rows, dp, sp});
}

static bool host_range_is_pinned(const void *p, size_t bytes)
{
    if (!p || !bytes)
        return false;
    const unsigned char *ends[2] = {(const unsigned char *)p, (const unsigned char *)p + bytes - 1};
    for (const unsigned char *q : ends) {
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof at);
        if (hipPointerGetAttributes(&at, q) != hipSuccess) {
            (void)hipGetLastError();  // plain malloc memory: not an error of ours
            return false;
        }
        if (at.type != hipMemoryTypeHost)
            return false;
    }
    return true;
}

static int stage_alloc(lumahip_ctx *c, lumahip_ctx::Stage &st, size_t bytes = XFER_CHUNK)
{
    if (!st.h) {
        // on the GPU's NUMA node: the calling thread's memory policy says where, hipHostMallocNumaUser makes the runtime follow it
        numa_resolve(c);
        bool placed = false;
        if (c->numa_node >= 0 && c->numa_mode != 3 && numa_prefer_node(c->numa_node)) {
            placed = hipHostMalloc((void **)&st.h, bytes, hipHostMallocNumaUser) == hipSuccess;
            if (!numa_prefer_node(-1)) {
                // the caller's memory policy could not be put back: its later allocations would silently prefer the GPU's node.
                // Say so, and stop placing rings for this context (the rings already made stay where they are)
                c->numa_mode = 0;
                c->numa_node = -1;
                (void)fail(c, LUMAHIP_ERR_STATE, "set_mempolicy could not restore the calling thread's memory policy after placing a "
                                                 "staging ring; NUMA placement is off for this context from here on");
                if (placed)
                    (void)hipHostFree(st.h);
                st.h = nullptr;
                return LUMAHIP_ERR_STATE;
            }
            if (!placed) {
                st.h = nullptr;
                (void)hipGetLastError();
            }
        }
        if (!placed)
            HIPCHK(c, hipHostMalloc((void **)&st.h, bytes, hipHostMallocDefault));
        if (!st.ev)
            HIPCHK(c, hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
    }
    return LUMAHIP_OK;
}

// An upload chunk is free again once the DMA that read it has completed.
// A download chunk is free again once its DMA has landed AND its bytes have been copied out to the caller's pageable
// memory; the copy happens here, i.e. lazily, when the ring comes round to the chunk again or when a call drains what is
// still in flight (d2h_flush).  The calling thread therefore never waits for a download it has only just queued: it goes
// on staging the next upload, which is what keeps the copy engine busy in the batched entry points (pageable frames:
// 3.1 -> 4.1 Gpixel/s once the fetch of frame i-1 stopped blocking the staging of frame i+1).  A context-owned thread that
// empties the chunks concurrently was built and measured as well: +2 % on that path, -5 % on the download-heavy decode
// calls (it copies single-threaded where this thread uses the copy threads), so it was not kept (profiles/r03_hostfed_sweep.txt).
static int stage_ready(lumahip_ctx *c, lumahip_ctx::Stage &st, size_t bytes = XFER_CHUNK)
{
    if (int rc = stage_alloc(c, st, bytes))
        return rc;
    if (st.pending) {
        HIPCHK(c, hipEventSynchronize(st.ev));
        st.pending = false;
        if (st.out) {   // (a pending download chunk; upload chunks have nowhere to go)
            staged_copy(c, st.out, st.out_pitch, st.h, st.chunk_pitch, st.width, st.rows);
            st.out = nullptr;
        }
    }
    return LUMAHIP_OK;
}

// Every device -> host chunk still in flight: wait for it and copy it out (chunks are in issue order, oldest first).  With
// `upto` (the pop of a pushed frame): only the chunks of pushed frames up to that sequence number and those of plain calls
static int d2h_flush(lumahip_ctx *c, const unsigned *upto = nullptr)
{
    for (int i = 0; i < lumahip_ctx::N_STAGE_DN; i++) {
        lumahip_ctx::Stage &st = c->stage_dn[(c->dn_next + i) % lumahip_ctx::N_STAGE_DN];
        if (st.h && st.pending && (!upto || (int)(st.tag - (*upto + 1)) <= 0))   // (tags are sequence number + 1; 0 = a chunk of a plain call: always due)
            if (int rc = stage_ready(c, st, c->dn_chunk))
                return rc;
    }
    return LUMAHIP_OK;
}

// Error paths: download chunks that are still pending point into the CALLER's memory (st.out).  A call that fails must not
// leave them behind -- a later flush, or the ring coming round, would copy into buffers the caller may have freed by then.
// d2h_drop waits for the DMA of every such chunk (all of them, or those with one tag: 0 = the plain calls, sequence number + 1 =
// one pushed frame, so that a failing plain call leaves the chunks of frames pushed earlier alone) and forgets it without copying; DnGuard does that on every exit of a scope that has not been told the downloads were completed or handed over.
static void d2h_drop(lumahip_ctx *c, bool all, unsigned tag)
{
    for (auto &st : c->stage_dn)
        if (st.h && st.pending && (all || st.tag == tag)) {
            if (st.ev)
                (void)hipEventSynchronize(st.ev);
            st.pending = false;
            st.out = nullptr;
        }
}
struct DnGuard {
    lumahip_ctx *c;
    bool all;
    unsigned tag;
    bool armed = true;
    ~DnGuard()
    {
        if (!armed)
            return;
        if (c->s_d2h)
            (void)hipStreamSynchronize(c->s_d2h);
        d2h_drop(c, all, tag);
    }
};

// The pipelined encode paths queue a whole frame's planes for download and go back to staging the next upload; that only
// works while the ring of download chunks holds the frame (five chunks of 8 MiB for a 4K frame's 25 MB, eight are there).
// The planes of an 8K frame are 99.5 MB: thirteen such chunks -- the ring came round to chunks of the SAME frame, the host sat
// waiting for its kernel, and the pipelined paths were slower than the synchronous one (3.35 against 3.55 Gpixel/s).  So the
// download chunks grow with the frame (a fifth of the planes, at most 32 MiB each); they are re-allocated only when nothing is
// in flight.
static int dn_chunks_for(lumahip_ctx *c, size_t planes_bytes)
{
    size_t want = ((planes_bytes / 5 + ((size_t)1 << 20) - 1) >> 20) << 20;
    want = std::min(std::max(want, XFER_CHUNK), (size_t)32 << 20);
    if (want <= c->dn_chunk)
        return LUMAHIP_OK;
    if (int rc = d2h_flush(c))
        return rc;
    for (auto &st : c->stage_dn)
        if (st.h) {
            (void)hipHostFree(st.h);
            st.h = nullptr;   // (the event stays; stage_alloc makes the new buffer on first use)
        }
    c->dn_chunk = want;
    return LUMAHIP_OK;
}

// The two ends of a staged upload.  up_chunk_take: the next upload chunk of the ring, free again, and *cap = how many bytes of it
// this call fills.  The first chunks of a call are small (1, 2, 4 MiB, then whole chunks): the copy engine starts after 15 us of
// staging instead of after the 110 us a whole chunk takes to fill, and nothing of that lead is lost later because the
// DMA of a chunk (150 us) takes longer than filling the next one.
static int up_chunk_take(lumahip_ctx *c, lumahip_ctx::Stage **st, size_t *cap)
{
    *st = &c->stage_up[c->up_next++ % lumahip_ctx::N_STAGE];
    if (int rc = stage_ready(c, **st))
        return rc;
    *cap = XFER_CHUNK;
    if (c->up_ramp < 3)
        *cap = std::min(*cap, (size_t)1 << (20 + c->up_ramp++));
    return LUMAHIP_OK;
}
// up_chunk_queue: the DMA of the chunk's first `bytes` bytes to `dst` on `s`, and the event that frees the chunk
static int up_chunk_queue(lumahip_ctx *c, lumahip_ctx::Stage &st, void *dst, size_t bytes, hipStream_t s)
{
    HIPCHK(c, hipMemcpyAsync(dst, st.h, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(st.ev, s));
    st.pending = true;
    return LUMAHIP_OK;
}

// rows x width bytes, host pitch hp, device pitch dp.  Returns once the copies are queued on `s` (the caller's buffer
// is no longer needed if it was pageable: it has been copied into the staging chunks).
static int xfer_h2d_2d(lumahip_ctx *c, void *dst, size_t dp, const void *src, size_t hp, size_t width, size_t rows, hipStream_t s)
{
    if (!width || !rows)
        return LUMAHIP_OK;
    if (host_range_is_pinned(src, (rows - 1) * hp + width)) {
        if (dp == width && hp == width)
            HIPCHK(c, hipMemcpyAsync(dst, src, width * rows, hipMemcpyHostToDevice, s));
        else
            HIPCHK(c, hipMemcpy2DAsync(dst, dp, src, hp, width, rows, hipMemcpyHostToDevice, s));
        return LUMAHIP_OK;
    }
    // staged: the device side is written as whole rows of dp bytes (the padding between rows belongs to the context's
    // own buffers), so that one chunk is one contiguous DMA
    const bool flat = (dp == width && hp == width);
    if (!flat && dp > XFER_CHUNK)
        return fail(c, LUMAHIP_ERR_ARG, "row pitch %zu exceeds the staging chunk", dp);
    const size_t total = flat ? width * rows : rows;                 // bytes or rows
    for (size_t done = 0; done < total;) {
        lumahip_ctx::Stage *st;
        size_t cap;
        if (int rc = up_chunk_take(c, &st, &cap))
            return rc;
        const size_t per = flat ? cap : std::max<size_t>(1, cap / dp);   // bytes or rows per chunk
        const size_t n = total - done < per ? total - done : per;
        size_t bytes;
        if (flat) {
            staged_copy(c, st->h, 0, (const unsigned char *)src + done, 0, n, 1);
            bytes = n;
        } else {
            staged_copy(c, st->h, dp, (const unsigned char *)src + done * hp, hp, width, n);
            bytes = (n - 1) * dp + width;
        }
        if (int rc = up_chunk_queue(c, *st, (unsigned char *)dst + done * (flat ? 1 : dp), bytes, s))
            return rc;
        done += n;
    }
    return LUMAHIP_OK;
}

namespace lhost {

int xfer_h2d(lumahip_ctx *c, void *dst, const void *src, size_t bytes, hipStream_t s)
{
    return xfer_h2d_2d(c, dst, bytes, src, bytes, bytes, 1, s);
}

}

// Host floats -> device halves: the half upload.  The reference's LumaFrame is float, but its EXR reader fills it with widened
// binary16 values (src/exr_interface.cpp:77-146); such a frame crosses PCIe in 6 instead of 12 bytes per pixel, and the encode
// kernels instantiated for binary16 input (k_encode<., ., 4, 3, IN16>) widen it back exactly.  The copy threads convert while
// they stage (reading 12 B and writing 6 B per pixel moves less memory than the plain staging copy) and check every value's
// round trip; *exact = false as soon as a chunk holds anything that is not a half -- nothing of that chunk has been queued then,
// and the caller uploads the frame (or band) as floats instead.  Pinned or pageable `src` alike: the CPU reads it either way.
static int xfer_h2d_f16(lumahip_ctx *c, void *dst_halves, const float *src, size_t nfloats, hipStream_t s, bool *exact)
{
    *exact = true;
    lumahip_copy_pool *const pool = copy_pool(c);
    for (size_t done = 0; done < nfloats;) {
        lumahip_ctx::Stage *st;
        size_t cap;   // bytes of halves
        if (int rc = up_chunk_take(c, &st, &cap))
            return rc;
        const size_t n = std::min(nfloats - done, cap / 2);
        const bool ok = pool ? pool->copy_to_half(reinterpret_cast<uint16_t *>(st->h), src + done, n)
                             : lh::convert_f32_to_f16_checked(src + done, reinterpret_cast<uint16_t *>(st->h), n);
        if (!ok) {
            *exact = false;
            return LUMAHIP_OK;
        }
        if (int rc = up_chunk_queue(c, *st, (unsigned char *)dst_halves + done * 2, n * 2, s))
            return rc;
        done += n;
    }
    return LUMAHIP_OK;
}

// Whether this call tries the half upload (lumahip_tune "half_upload": 0 never, 1 while the frames hold halves, 2 always try).
// A frame that turns out to hold other values costs the conversion of its first chunks for nothing, so after one such frame
// the next 16 go up as floats before one is tried again, the pause doubling up to 1024 frames while the misses continue.
static bool in16_try(lumahip_ctx *c, unsigned w, bool wants_float_frame)
{
    if (c->in16_mode == 0 || wants_float_frame || !lh::f16c_available() || !encode_supports_in16(c, w))
        return false;
    if (c->in16_mode == 2)
        return true;
    if (c->in16_backoff > 0) {
        c->in16_backoff--;
        return false;
    }
    return true;
}
static void in16_result(lumahip_ctx *c, bool exact)
{
    if (exact) {
        c->in16_frames++;
        c->in16_backoff_len = 0;
    } else {
        c->in16_fallbacks++;
        c->in16_backoff_len = c->in16_backoff_len ? std::min(2 * c->in16_backoff_len, 1024) : 16;
        c->in16_backoff = c->in16_backoff_len;
    }
}

// `count` spans of n floats each, span i at element off + i * stride of BOTH the caller's frame `src` and the device frame `dst`
// (one whole packed frame: one span; a row band: the band's rows of each of the three channels)
struct FloatSpans { float *dst; const float *src; size_t off, n, count, stride; };

// The spans go up on `s`: as halves -- at the same element offsets of dst read as uint16_t -- if `try16` and every value is one,
// else as floats; *as16 says which.  A span that holds other values ends the attempt (nothing of its chunk has been queued) and
// ALL spans go up as floats, after before_floats(): what the caller has to do before floats overwrite the halves already queued.
template <typename BeforeFloats>
static int upload_floats(lumahip_ctx *c, const FloatSpans &sp, hipStream_t s, bool try16, bool *as16, BeforeFloats before_floats)
{
    int rc = LUMAHIP_OK;
    *as16 = try16;
    for (size_t i = 0; i < sp.count && rc == LUMAHIP_OK && *as16; i++)
        rc = xfer_h2d_f16(c, reinterpret_cast<uint16_t *>(sp.dst) + sp.off + i * sp.stride, sp.src + sp.off + i * sp.stride, sp.n, s, as16);
    if (rc || *as16)
        return rc;
    if (try16 && (rc = before_floats()))
        return rc;
    for (size_t i = 0; i < sp.count && rc == LUMAHIP_OK; i++)
        rc = xfer_h2d(c, sp.dst + sp.off + i * sp.stride, sp.src + sp.off + i * sp.stride, sp.n * sizeof(float), s);
    return rc;
}

// Device -> host.  Pinned destination: queued on `s`, the caller synchronises.  Pageable destination: the data goes through
// the ring of pinned chunks; with `deferred` false it is in `dst` when the call returns (everything queued on `s` before it has
// completed by then), with `deferred` true the last chunks may still be in flight and d2h_flush() completes them -- which lets
// the DMA of one piece overlap the copy-out of the previous one ACROSS calls (the row bands of the host entry points).
static int xfer_d2h_2d(lumahip_ctx *c, void *dst, size_t hp, const void *src, size_t dp, size_t width, size_t rows, hipStream_t s,
                       bool deferred = false)
{
    if (!width || !rows)
        return LUMAHIP_OK;
    if (host_range_is_pinned(dst, (rows - 1) * hp + width)) {
        if (dp == width && hp == width)
            HIPCHK(c, hipMemcpyAsync(dst, src, width * rows, hipMemcpyDeviceToHost, s));
        else
            HIPCHK(c, hipMemcpy2DAsync(dst, hp, src, dp, width, rows, hipMemcpyDeviceToHost, s));
        return LUMAHIP_OK;
    }
    const bool flat = (dp == width && hp == width);
    if (!flat && dp > c->dn_chunk)
        return fail(c, LUMAHIP_ERR_ARG, "row pitch %zu exceeds the staging chunk", dp);
    const size_t total = flat ? width * rows : rows;
    const size_t per = flat ? c->dn_chunk : c->dn_chunk / dp;
    for (size_t done = 0; done < total;) {
        lumahip_ctx::Stage &st = c->stage_dn[c->dn_next++ % lumahip_ctx::N_STAGE_DN];
        if (int rc = stage_ready(c, st, c->dn_chunk))   // the chunk this ring slot carried N_STAGE_DN chunks ago has been emptied
            return rc;
        const size_t n = total - done < per ? total - done : per;
        const size_t bytes = flat ? n : (n - 1) * dp + width;
        HIPCHK(c, hipMemcpyAsync(st.h, (const unsigned char *)src + done * (flat ? 1 : dp), bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipEventRecord(st.ev, s));
        st.out = (unsigned char *)dst + done * (flat ? 1 : hp);   // what stage_ready copies out: one span of n bytes, or n rows
        st.out_pitch = flat ? 0 : hp;
        st.chunk_pitch = flat ? 0 : dp;
        st.width = flat ? n : width;
        st.rows = flat ? 1 : n;
        st.tag = c->d2h_tag;
        st.pending = true;
        done += n;
    }
    return deferred ? LUMAHIP_OK : d2h_flush(c);
}

namespace lhost {

int xfer_d2h(lumahip_ctx *c, void *dst, const void *src, size_t bytes, hipStream_t s)
{
    return xfer_d2h_2d(c, dst, bytes, src, bytes, bytes, 1, s);
}

static int xfer_d2h_deferred(lumahip_ctx *c, void *dst, const void *src, size_t bytes, hipStream_t s)
{
    return xfer_d2h_2d(c, dst, bytes, src, bytes, bytes, 1, s, true);
}

// a few floats from the device: through the pinned scratch, synchronous
int read_small(lumahip_ctx *c, float *dst, const float *src_dev, int n, hipStream_t s)
{
    if (!c->h_small)
        HIPCHK(c, hipHostMalloc((void **)&c->h_small, 64 * sizeof(float), hipHostMallocDefault));
    HIPCHK(c, hipMemcpyAsync(c->h_small, src_dev, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    memcpy(dst, c->h_small, (size_t)n * sizeof(float));
    return LUMAHIP_OK;
}

int ensure(lumahip_ctx *c, void **p, size_t *cap, size_t need)
{
    if (*cap >= need)
        return LUMAHIP_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HIPCHK(c, hipMalloc(p, need));
    *cap = need;
    return LUMAHIP_OK;
}

}  // namespace lhost

struct PlaneLayout {
    bool sub;           // 4:2:0: the colour planes have half the rows and half the columns
    int rows[3];
    int row_bytes[3];
    size_t off[3];
    size_t total;
};

static void plane_layout(PlaneLayout &L, unsigned w, unsigned h, int profile, const int stride[3])
{
    const bool sub = (profile == 0 || profile == 2);
    const int bps = profile > 1 ? 2 : 1;
    size_t off = 0;
    L.sub = sub;
    for (int p = 0; p < 3; p++) {
        const int pw = (p && sub) ? (int)(w + 1) / 2 : (int)w;
        const int ph = (p && sub) ? (int)(h + 1) / 2 : (int)h;
        L.rows[p] = ph;
        L.row_bytes[p] = pw * bps;
        L.off[p] = off;
        off += ((size_t)ph * stride[p] + 255) & ~(size_t)255;
    }
    L.total = off;
}

// the first plane that is null or whose stride is below its row bytes; -1: none
static int bad_plane(const PlaneLayout &L, const unsigned char *const planes[3], const int stride[3])
{
    for (int p = 0; p < 3; p++)
        if (!planes[p] || stride[p] < L.row_bytes[p])
            return p;
    return -1;
}

// frame rows -> rows of plane p (frames have even heights and bands start at multiples of 16 rows: nothing is cut off)
static unsigned plane_row(const PlaneLayout &L, int p, unsigned r) { return (p && L.sub) ? r / 2 : r; }

// dp[] = the three code planes in the device buffer `base` (the context's or a slot's), from frame row r0 on
static void device_planes(unsigned char *dp[3], unsigned char *base, const PlaneLayout &L, const int stride[3], unsigned r0 = 0)
{
    for (int p = 0; p < 3; p++)
        dp[p] = base + L.off[p] + (size_t)plane_row(L, p, r0) * stride[p];
}

// Rows [r0, r0 + rows) of the frame, code plane p: caller's plane -> device plane (dp[]: the whole planes) ...
static int plane_h2d(lumahip_ctx *c, unsigned char *const dp[3], const unsigned char *const planes[3], const int stride[3], const PlaneLayout &L,
                     int p, unsigned r0, unsigned rows, hipStream_t s)
{
    const size_t off = (size_t)plane_row(L, p, r0) * stride[p];
    return xfer_h2d_2d(c, dp[p] + off, stride[p], planes[p] + off, stride[p], L.row_bytes[p], plane_row(L, p, rows), s);
}
// ... and the three device planes -> the caller's (deferred: see xfer_d2h_2d)
static int planes_d2h(lumahip_ctx *c, unsigned char *const planes[3], unsigned char *const dp[3], const int stride[3], const PlaneLayout &L,
                      unsigned r0, unsigned rows, hipStream_t s, bool deferred)
{
    for (int p = 0; p < 3; p++) {
        const size_t off = (size_t)plane_row(L, p, r0) * stride[p];
        if (int rc = xfer_d2h_2d(c, planes[p] + off, stride[p], dp[p] + off, stride[p], L.row_bytes[p], plane_row(L, p, rows), s, deferred))
            return rc;
    }
    return LUMAHIP_OK;
}

// What the single-frame host calls open with: the arguments checked, the plane layout, the context's staging buffers large
// enough for one w x h frame of floats (binary16 frames share them) and its planes, dp[] = the device planes
static int frame_staging(lumahip_ctx *c, const void *frame, const unsigned char *const planes[3], const int stride[3], unsigned w,
                         unsigned h, int profile, int cs_eff, PlaneLayout &L, unsigned char *dp[3])
{
    if (!c || !frame || !planes || !stride)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    int rc = check_geom(c, w, h, profile, cs_eff);
    if (rc)
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    c->up_ramp = 0;   // (per call, like the push; the frames of a batched call share one ramp)
    plane_layout(L, w, h, profile, stride);
    const int p = bad_plane(L, planes, stride);
    if (p >= 0)
        return fail(c, LUMAHIP_ERR_ARG, "plane %d: null or stride %d < row bytes %d", p, stride[p], L.row_bytes[p]);
    if ((rc = ensure(c, (void **)&c->d_frame, &c->d_frame_cap, (size_t)3 * w * h * sizeof(float))))
        return rc;
    if ((rc = ensure(c, (void **)&c->d_planes, &c->d_planes_cap, L.total)))
        return rc;
    device_planes(dp, c->d_planes, L, stride);
    return LUMAHIP_OK;
}

// The reference warns when its (sequentially summed) mean luminance is <= 1.  That fp32 sum is far from the true sum on
// large frames: once the running sum S is large, addends below ulp(S)/2 vanish and the rest are rounded to multiples of
// ulp(S) (measured: -0.2 % at 1080p, several % at 4K on wide-range content), whereas the kernels' statistic (per-wave
// partial sums) is accurate to ~1e-6.  For N <= 2^25 non-negative values (up to 8K frames) S stays below N * 4 around the
// threshold, i.e. ulp(S)/2 <= 2, so the two can only disagree about `<= 1` when the accurate mean lies in [0.25, 4]: inside
// that band the host entry points replace the statistic by the reference's exact value (k_seq_sum), outside it the decision
// is the same either way.  The argument needs both premises, so frames beyond 2^25 pixels and frames whose channel 0 has
// negative values (possible for CS_RGB and the pack-only entry points: cancellation, no bound) always take the exact sum.
static bool mean_needs_reference_sum(float mean, float minimum, unsigned w, unsigned h)
{
    if ((size_t)w * h > ((size_t)1 << 25) || !(minimum >= 0.0f))
        return true;
    return mean >= 0.25f && mean <= 4.0f;
}

// ---- the 3-stage pipeline every host-fed loop runs ------------------------------------------------------------------------
// Three streams: stage t goes up on s_h2d | stage t's kernel runs on s_kern behind the upload's event | stage t-1 comes down on
// s_d2h behind its kernel's event.  A stage is a frame in one of the three device slots (the batched calls; the stream push /
// pop, where the loop is carried across calls) or a row band of one frame in the context's staging buffers.  With pinned caller
// memory (lumahip_host_register) the two copy directions overlap as well and the rate approaches the PCIe H2D rate.
static int pipe_streams(lumahip_ctx *c)
{
    if (!c->s_h2d) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->s_h2d, hipStreamNonBlocking));
        HIPCHK(c, hipStreamCreateWithFlags(&c->s_kern, hipStreamNonBlocking));
        HIPCHK(c, hipStreamCreateWithFlags(&c->s_d2h, hipStreamNonBlocking));
    }
    return LUMAHIP_OK;
}

struct PipeStage {
    hipEvent_t h2d, kern;
    hipEvent_t d2h;    // null for a row band: nothing waits for a band's download but the end of the call
    float *d_stats;    // where the stage's encode kernel leaves its statistics triple
    bool reuses;       // its device buffers were those of the stage three before it (slots, from the fourth frame on)
};
static PipeStage slot_stage(const lumahip_ctx::Slot &sl, unsigned seq) { return {sl.h2d, sl.kern, sl.d2h, sl.d_stats, seq >= 3}; }
static PipeStage band_stage(lumahip_ctx *c, unsigned k) { return {c->band_h2d[k], c->band_kern[k], nullptr, c->d_band_stats + 3 * k, false}; }

// The front half of a stage: upload() queues the stage's input on s_h2d, launch() its kernel on s_kern.  A failing event call
// is reported like a failing transfer or launch (the batched and push forms used to discard those results).
template <typename Upload, typename Launch>
static int pipe_issue(lumahip_ctx *c, const PipeStage &st, Upload &&upload, Launch &&launch)
{
    if (st.reuses) {
        // The previous occupant's kernel must have consumed the stage's input buffer, its download must have drained the output
        // buffer.  (Stream push: that frame was popped long ago and both are done, but the streams still have to be told.)
        HIPCHK(c, hipStreamWaitEvent(c->s_h2d, st.kern, 0));
        HIPCHK(c, hipStreamWaitEvent(c->s_kern, st.d2h, 0));
    }
    if (int rc = upload())
        return rc;
    HIPCHK(c, hipEventRecord(st.h2d, c->s_h2d));
    HIPCHK(c, hipStreamWaitEvent(c->s_kern, st.h2d, 0));
    if (int rc = launch())
        return rc;
    HIPCHK(c, hipEventRecord(st.kern, c->s_kern));
    return LUMAHIP_OK;
}

// The back half: download() queues the stage's output on s_d2h, behind its kernel.  The downloads are DEFERRED: pageable
// destinations are copied out of the staging chunks when the ring comes round to them, by pipe_drain or by the pop -- not here,
// where it would hold up the staging of the next stage's upload (see stage_ready).  h_stats: pinned, where the statistics
// triple goes along (nullptr: not wanted).
template <typename Download>
static int pipe_fetch(lumahip_ctx *c, const PipeStage &st, Download &&download, float *h_stats)
{
    HIPCHK(c, hipStreamWaitEvent(c->s_d2h, st.kern, 0));
    if (int rc = download())
        return rc;
    if (h_stats)
        HIPCHK(c, hipMemcpyAsync(h_stats, st.d_stats, 3 * sizeof(float), hipMemcpyDeviceToHost, c->s_d2h));
    if (st.d2h)
        HIPCHK(c, hipEventRecord(st.d2h, c->s_d2h));
    return LUMAHIP_OK;
}

// The end of a pipelined call, after an error as well (rc: the error so far; nothing may stay pending): the download chunks
// still in flight are copied out -- only then is the guard told that nothing points into the caller's memory any more -- and the
// three streams run dry.  Returns the first error.
static int pipe_drain(lumahip_ctx *c, DnGuard &guard, int rc)
{
    if (int r = d2h_flush(c))
        rc = rc ? rc : r;
    else
        guard.armed = false;
    for (hipStream_t s : {c->s_h2d, c->s_kern, c->s_d2h}) {
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess && rc == LUMAHIP_OK)
            rc = fail(c, LUMAHIP_ERR_HIP, "hipStreamSynchronize failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    }
    return rc;
}

// n stages, one behind: stage t is uploaded and launched BEFORE stage t-1 is fetched, the last one is fetched after the loop.
// stage_of(t): its events; upload(t), launch(t, stage), download(t): its bodies; h_stats as in pipe_fetch, 3 floats per stage.
// Every failure ends the loop and goes through the drain; if the drain itself cannot empty the chunks, the guard drops them.
template <typename StageOf, typename Upload, typename Launch, typename Download>
static int pipe_run(lumahip_ctx *c, unsigned n, StageOf stage_of, Upload upload, Launch launch, Download download, float *h_stats = nullptr)
{
    DnGuard guard{c, false, 0};   // a failing exit drops the download chunks still pointing at the caller's buffers
    auto fetch_stage = [&](unsigned t) {
        return pipe_fetch(c, stage_of(t), [&] { return download(t); }, h_stats ? h_stats + 3 * (size_t)t : nullptr);
    };
    int rc = LUMAHIP_OK;
    for (unsigned t = 0; t < n && rc == LUMAHIP_OK; t++) {
        const PipeStage st = stage_of(t);
        rc = pipe_issue(c, st, [&] { return upload(t); }, [&] { return launch(t, st); });
        if (rc == LUMAHIP_OK && t >= 1)
            rc = fetch_stage(t - 1);
    }
    if (rc == LUMAHIP_OK)
        rc = fetch_stage(n - 1);
    return pipe_drain(c, guard, rc);
}

// ---- row bands ------------------------------------------------------------------------------------------------------------
// One host frame per call is PCIe time: 99.5 MB up at ~56 GB/s (1.76 ms), 30 us of kernel, 24.9 MB down (0.45 ms); done one
// after the other that is 2.2 ms pinned and more staged (profiles/r03_hostfed_lab.txt).  Rows are independent (pairs of rows
// in 4:2:0), so a large frame is cut into `host_bands` bands of rows: band k+1 goes up while band k is transformed and band
// k-1 comes down -- the link is full duplex -- and the call is bound by the upload plus whatever is left to do for the LAST
// band once its rows have arrived (its kernel, its download, the copy out of the staging chunks).  The bands therefore
// TAPER: each is `band_taper` % of the previous one (default 70: 39.5 / 27.6 / 19.3 / 13.5 % of the rows for four bands), so that
// tail is an eighth of the frame instead of a quarter (rocprofv3 timeline of the uniform split: 0.5 ms of 2.67 ms per
// pageable 4K frame after the last upload chunk; profiles/r03_hostfed_timeline.txt).  A download still fits under the next
// band's upload: it moves a quarter of the bytes.  Bands are multiples of 16 rows (whole tiles of every kernel variant); the
// pixel arithmetic does not depend on the split.
static int band_plan(const lumahip_ctx *c, unsigned w, unsigned h, unsigned r0[lumahip_ctx::MAX_BANDS + 1])
{
    int nb = c->host_bands;
    // small frames are latency, not bandwidth: up to 1920x1080 one piece is as fast or faster (registered frames +10 %, pageable
    // +-0; profiles/r03_hostfed_sweep.txt), from 2560x1440 on the bands win (pageable +12 %)
    if ((size_t)w * h < (size_t)3 << 20 || nb < 2)
        nb = 1;
    const double q = c->band_taper / 100.0;
    double wsum = 0.0, wk = 1.0;
    for (int k = 0; k < nb; k++, wk *= q)
        wsum += wk;
    unsigned row = 0;
    int k = 0;
    wk = 1.0;
    r0[0] = 0;
    for (int i = 0; i < nb && row < h; i++, wk *= q) {
        unsigned rows = (unsigned)(h * (wk / wsum) + 0.5);
        rows = (rows + 15) & ~15u;
        if (rows < 64)
            rows = 64;
        if (i == nb - 1 || row + rows > h || h - (row + rows) < 64)   // the last band takes what is left
            rows = h - row;
        row += rows;
        r0[++k] = row;
    }
    return k;   // number of bands; band i = rows [r0[i], r0[i+1])
}

// what a banded call opens with: the pipeline's streams, the bands' events and statistics, and the context's stream run dry --
// the bands run on the pipeline streams, after everything queued so far
static int band_prepare(lumahip_ctx *c, int nb)
{
    if (int rc = pipe_streams(c))
        return rc;
    for (int k = 0; k < nb; k++)
        if (!c->band_h2d[k]) {
            HIPCHK(c, hipEventCreateWithFlags(&c->band_h2d[k], hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->band_kern[k], hipEventDisableTiming));
        }
    if (!c->d_band_stats)
        HIPCHK(c, hipMalloc(&c->d_band_stats, lumahip_ctx::MAX_BANDS * 3 * sizeof(float)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LUMAHIP_OK;
}

// rgb: the caller's frame, floats or -- elem == F16, lumahip_encode_frame_host_f16 -- halves by type.  Halves by type go up as
// they are, 6 B per pixel, in one piece on the context's stream: no row bands, no round-trip test, none of the half upload's
// bookkeeping (in16_try / in16_result)
static int encode_frame_host_impl(lumahip_ctx *c, const void *rgb_any, Elem elem, unsigned w, unsigned h, float sc, int profile,
                                  unsigned char *const planes[3], const int stride[3], float *mean_lum,
                                  float *transformed_out, int cs_eff)
{
    PlaneLayout L;
    unsigned char *dp[3];
    int rc = frame_staging(c, rgb_any, planes, stride, w, h, profile, cs_eff, L, dp);
    if (rc)
        return rc;
    if (!c->d_stats)
        HIPCHK(c, hipMalloc(&c->d_stats, 3 * sizeof(float)));
    const bool typed16 = elem == Elem::F16;
    const float *const rgb = typed16 ? nullptr : static_cast<const float *>(rgb_any);
    const size_t nfl = (size_t)3 * w * h;
    const size_t n1 = (size_t)w * h;
    unsigned band0[lumahip_ctx::MAX_BANDS + 1];
    const int nb = typed16 ? 1 : band_plan(c, w, h, band0);
    float st[3] = {0.0f, __builtin_inff(), -__builtin_inff()};
    // Half upload (xfer_h2d_f16): tried unless the caller wants the transformed FLOAT frame back.  frame16: every band so far went
    // up as halves; mixed: some did and then a band held other values -- the device frame is then not usable as a whole.
    // (nor for frames that are already colour-transformed -- lumahip_pack_frame_host: such values are never halves)
    bool use16 = !typed16 && in16_try(c, w, transformed_out != nullptr || cs_eff == CS_PACK), frame16 = use16 || typed16, mixed = false;
    const bool tried16 = use16;
    uint16_t *const d16 = reinterpret_cast<uint16_t *>(c->d_frame);   // the staging frame when it holds halves: same element offsets
    auto staged = [&]() -> SrcFrames { return frame16 ? packed_frames<const uint16_t>(d16, nfl, 1, w, h) : packed_frames<const float>(c->d_frame, nfl, 1, w, h); };
    // the caller's floats (the whole frame, or a band of it) into the staging frame; once a piece has gone up as floats, so do the rest
    auto upload = [&](const FloatSpans &sp, hipStream_t s, auto before_floats) {
        bool as16;
        const int r = upload_floats(c, sp, s, use16, &as16, before_floats);
        use16 = frame16 = use16 && as16;
        return r;
    };
    if (nb > 1) {
        if ((rc = band_prepare(c, nb)))
            return rc;
        rc = pipe_run(
            c, nb, [&](unsigned k) { return band_stage(c, k); },
            [&](unsigned k) {
                const unsigned r0 = band0[k], rows = band0[k + 1] - r0;
                return upload({c->d_frame, rgb, (size_t)r0 * w, (size_t)rows * w, 3, n1}, c->s_h2d, [&] {
                    // this band holds values that are not halves: it and the rest of the frame go up as floats -- into the same
                    // buffer, at float offsets, which the kernels of the earlier bands may still be reading as halves: wait for them
                    mixed = k > 0;
                    HIPCHK(c, hipStreamSynchronize(c->s_kern));
                    return (int)LUMAHIP_OK;
                });
            },
            [&](unsigned k, const PipeStage &bs) {
                const unsigned r0 = band0[k], rows = band0[k + 1] - r0;
                unsigned char *bp[3];
                device_planes(bp, c->d_planes, L, stride, r0);
                return encode_frames_device_impl(c, row_band(staged(), r0, rows), sc, {bp, stride, NO_PFS, profile}, bs.d_stats,
                                                 {cs_eff, c->s_kern, false, HalfSource::Upload});
            },
            [&](unsigned k) { return planes_d2h(c, planes, dp, stride, L, band0[k], band0[k + 1] - band0[k], c->s_d2h, true); });
        if (rc)
            return rc;
        float bs[lumahip_ctx::MAX_BANDS * 3];
        if ((rc = read_small(c, bs, c->d_band_stats, 3 * nb, c->stream)))
            return rc;
        for (int k = 0; k < nb; k++) {
            st[0] += bs[3 * k];
            st[1] = fminf(st[1], bs[3 * k + 1]);
            st[2] = fmaxf(st[2], bs[3 * k + 2]);
        }
    } else {
        // (a frame that turns out not to hold halves: nothing has been launched on them, the floats simply follow on the same stream)
        if ((rc = typed16 ? xfer_h2d(c, d16, rgb_any, nfl * sizeof(uint16_t), c->stream)
                          : upload({c->d_frame, rgb, 0, nfl, 1, 0}, c->stream, [] { return (int)LUMAHIP_OK; })))
            return rc;
        if ((rc = encode_frames_device_impl(c, staged(), sc, {dp, stride, NO_PFS, profile}, c->d_stats,
                                            {cs_eff, c->stream, false, typed16 ? HalfSource::Typed : HalfSource::Upload})))
            return rc;
        if ((rc = planes_d2h(c, planes, dp, stride, L, 0, h, c->stream, false)))
            return rc;
    }
    if (transformed_out) {
        rc = lumahip_transform_color_space_device(c, c->d_frame, nfl, 1, w, h, 1, sc);
        if (rc)
            return rc;
        if ((rc = xfer_d2h(c, transformed_out, c->d_frame, nfl * sizeof(float), c->stream)))
            return rc;
    }
    if (nb == 1 && (rc = read_small(c, st, c->d_stats, 3, c->stream)))  // synchronises the stream
        return rc;
    if (transformed_out)
        HIPCHK(c, hipStreamSynchronize(c->stream));
    if (tried16)
        in16_result(c, frame16);
    if (mean_lum) {
        *mean_lum = st[0] / (float)((int)w * (int)h);  // avg /= (w*h), src/luma_encoder.cpp:314
        if (mean_needs_reference_sum(*mean_lum, st[1], w, h)) {  // d_frame holds the caller's frame (as floats or as halves), or already its transformed version
            if (mixed && (rc = xfer_h2d(c, c->d_frame, rgb, nfl * sizeof(float), c->stream)))   // part halves, part floats: once more, whole
                return rc;
            return transformed_out ? seq_mean(c, c->d_frame, w, h, mean_lum)
                                   : mean_luminance_reference_impl(c, c->d_frame, frame16 ? Elem::F16 : Elem::F32, w, h, sc, cs_eff, mean_lum);
        }
    }
    return LUMAHIP_OK;
}

extern "C" int lumahip_encode_frame_host(lumahip_ctx *c, const float *rgb, unsigned w, unsigned h, float sc, int profile,
                                         unsigned char *const planes[3], const int stride[3], float *mean_lum,
                                         float *transformed_out)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    return encode_frame_host_impl(c, rgb, Elem::F32, w, h, sc, profile, planes, stride, mean_lum, transformed_out, c->q.cs);
}

// rgb_out: the caller's frame, floats or -- elem == F16, lumahip_decode_frame_host_f16 -- halves by type, which come down as
// the kernel wrote them, 6 B per pixel, in one piece on the context's stream
static int decode_frame_host_impl(lumahip_ctx *c, const unsigned char *const planes[3], const int stride[3], unsigned w,
                                  unsigned h, int profile, float sc, void *rgb_out, Elem elem, int cs_eff)
{
    PlaneLayout L;
    unsigned char *dp[3];
    int rc = frame_staging(c, rgb_out, planes, stride, w, h, profile, cs_eff, L, dp);
    if (rc)
        return rc;
    const size_t nfl = (size_t)3 * w * h;
    const size_t n1 = (size_t)w * h;
    unsigned band0[lumahip_ctx::MAX_BANDS + 1];
    const int nb = elem == Elem::F16 ? 1 : band_plan(c, w, h, band0);
    if (nb > 1) {
        float *const rgb_f = static_cast<float *>(rgb_out);
        if ((rc = band_prepare(c, nb)))
            return rc;
        return pipe_run(
            c, nb, [&](unsigned k) { return band_stage(c, k); },
            [&](unsigned k) {
                int r = LUMAHIP_OK;
                for (int p = 0; p < 3 && r == LUMAHIP_OK; p++)
                    r = plane_h2d(c, dp, planes, stride, L, p, band0[k], band0[k + 1] - band0[k], c->s_h2d);
                return r;
            },
            [&](unsigned k, const PipeStage &) {
                const unsigned r0 = band0[k], rows = band0[k + 1] - r0;
                unsigned char *bp[3];
                device_planes(bp, c->d_planes, L, stride, r0);
                return decode_impl(c, {bp, stride, NO_PFS, profile}, sc, row_band(packed_frames(c->d_frame, nfl, 1, w, h), r0, rows), {cs_eff, c->s_kern});
            },
            [&](unsigned k) {   // the band's rows of each channel; floats come down with the default chunk size (no dn_chunks_for)
                const size_t roff = (size_t)band0[k] * w, n = (size_t)(band0[k + 1] - band0[k]) * w;
                int r = LUMAHIP_OK;
                for (int ch = 0; ch < 3 && r == LUMAHIP_OK; ch++)
                    r = xfer_d2h_deferred(c, rgb_f + ch * n1 + roff, c->d_frame + ch * n1 + roff, n * sizeof(float), c->s_d2h);
                return r;
            });
    }
    for (int p = 0; p < 3; p++)
        if ((rc = plane_h2d(c, dp, planes, stride, L, p, 0, h, c->stream)))
            return rc;
    const DstFrames staged = elem == Elem::F16 ? packed_frames(reinterpret_cast<uint16_t *>(c->d_frame), nfl, 1, w, h)   // (the staging frame holding halves)
                                               : packed_frames(c->d_frame, nfl, 1, w, h);
    if ((rc = decode_impl(c, {dp, stride, NO_PFS, profile}, sc, staged, {cs_eff, c->stream})))
        return rc;
    if ((rc = xfer_d2h(c, rgb_out, c->d_frame, nfl * elem_size(elem), c->stream)))
        return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LUMAHIP_OK;
}

extern "C" int lumahip_decode_frame_host(lumahip_ctx *c, const unsigned char *const planes[3], const int stride[3],
                                         unsigned w, unsigned h, int profile, float sc, float *rgb_out)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    return decode_frame_host_impl(c, planes, stride, w, h, profile, sc, rgb_out, Elem::F32, c->q.cs);
}

// ---- the calls that stage code planes as INPUT: transcode, distortion, transcode distortion ---------------------------------
// One set of the caller's code planes and where it sits in the context's plane staging
struct StagedPlanes {
    const char *name;   // in error messages: "source ", "destination ", "given " or ""
    const unsigned char *const *planes;
    const int *stride;
    int profile;
    PlaneLayout L;
    unsigned char *dp[3];          // the device planes ...
    const unsigned char *cdp[3];   // ... and as a launch reads them
    SrcPlanes dev() const { return {cdp, stride, NO_PFS, profile}; }
};

// What those calls open with, after their null checks: the geometry against the target-side set `tgt`, the source set's profile and
// quantizer (src = nullptr: frames in, one set; tgt = nullptr too: a frame alone, quantizers = false), the layouts, d_planes large
// enough for [src][tgt].  quantizers = false: the sets are taken as they are (the plane-to-plane measures, the light level of a
// frame), neither quantizer is asked for.  tgt_scale 2 (the half-resolution transcode): w and h are multiples of 4 and the set `tgt`
// is laid out at (w/2) x (h/2); tgt_scale 4 (the quarter-resolution transcode): multiples of 8, and (w/4) x (h/4)
static int planes_staging(lumahip_ctx *c, unsigned w, unsigned h, StagedPlanes *src, StagedPlanes *tgt, bool quantizers = true, unsigned tgt_scale = 1)
{
    int rc = quantizers ? check_geom(c, w, h, tgt->profile, c->q.cs) : check_size(c, w, h);
    if (!rc && !quantizers && tgt)
        rc = check_profile(c, tgt->profile);
    if (rc)
        return rc;
    if (tgt_scale == 2 && ((w | h) & 3))
        return fail(c, LUMAHIP_ERR_ARG, "Invalid frame size %ux%u (half resolution: must be multiples of 4)", w, h);
    if (tgt_scale == 4 && ((w | h) & 7))
        return fail(c, LUMAHIP_ERR_ARG, "Invalid frame size %ux%u (quarter resolution: must be multiples of 8)", w, h);
    if (src && (src->profile < 0 || src->profile > 3))
        return fail(c, LUMAHIP_ERR_ARG, "source profile must be 0..3 (got %d)", src->profile);
    if (quantizers && src && !c->src.have)
        return fail(c, LUMAHIP_ERR_STATE, "source quantizer not set (call lumahip_set_source_quantizer first)");
    HIPCHK(c, hipSetDevice(c->device));
    c->up_ramp = 0;
    StagedPlanes *const sets[2] = {src, tgt};
    size_t total = 0;
    for (StagedPlanes *s : sets) {
        if (!s)
            continue;
        const unsigned sc = s == tgt ? tgt_scale : 1;
        plane_layout(s->L, w / sc, h / sc, s->profile, s->stride);
        const int p = bad_plane(s->L, s->planes, s->stride);
        if (p >= 0)
            return fail(c, LUMAHIP_ERR_ARG, "%splane %d: null or stride %d < row bytes %d", s->name, p, s->stride[p], s->L.row_bytes[p]);
        total += s->L.total;
    }
    if (total && (rc = ensure(c, (void **)&c->d_planes, &c->d_planes_cap, total)))
        return rc;
    size_t off = 0;
    for (StagedPlanes *s : sets) {
        if (!s)
            continue;
        device_planes(s->dp, c->d_planes + off, s->L, s->stride);
        for (int k = 0; k < 3; k++)
            s->cdp[k] = s->dp[k];
        off += s->L.total;
    }
    return LUMAHIP_OK;
}

static int planes_up(lumahip_ctx *c, const StagedPlanes &s, unsigned h)
{
    for (int k = 0; k < 3; k++)
        if (int rc = plane_h2d(c, s.dp, s.planes, s.stride, s.L, k, 0, h, c->stream))
            return rc;
    return LUMAHIP_OK;
}

// what the measuring calls close with: the 12 words, or a map's, down (synchronises the stream)
static int words_down(lumahip_ctx *c, uint64_t *out, size_t words)
{
    if (words == 12)
        return read_small(c, reinterpret_cast<float *>(out), reinterpret_cast<const float *>(c->d_arr), 24, c->stream);
    if (int rc = xfer_d2h(c, out, c->d_arr, words * sizeof(uint64_t), c->stream))
        return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LUMAHIP_OK;
}

// Source planes up, one transcode launch, destination planes down, synchronously on the context's stream; the context's plane
// staging holds both sets.  mean_lum as lumahip_encode_frame_host: the launch's statistic, replaced by the reference's
// sequential sum -- over channel 0 of the decoded and transformed frame, which only then is written, into the staging frame --
// in the cases where that call takes the exact sum too (mean_needs_reference_sum).
extern "C" int lumahip_transcode_frame_host(lumahip_ctx *c, const unsigned char *const src_planes[3], const int src_stride[3], int src_profile,
                                            float src_sc, unsigned w, unsigned h, unsigned char *const dst_planes[3], const int dst_stride[3],
                                            int dst_profile, float dst_sc, float *mean_lum)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!src_planes || !src_stride || !dst_planes || !dst_stride)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    StagedPlanes src{"source ", src_planes, src_stride, src_profile}, dst{"destination ", dst_planes, dst_stride, dst_profile};
    int rc = planes_staging(c, w, h, &src, &dst);
    if (rc)
        return rc;
    if (!c->d_stats)
        HIPCHK(c, hipMalloc(&c->d_stats, 3 * sizeof(float)));
    if ((rc = planes_up(c, src, h)) ||
        (rc = transcode_impl(c, src.dev(), src_sc, 1, w, h, {dst.dp, dst_stride, NO_PFS, dst_profile}, dst_sc, mean_lum ? c->d_stats : nullptr,
                             {c->stream, false})) ||
        (rc = planes_d2h(c, dst_planes, dst.dp, dst_stride, dst.L, 0, h, c->stream, false)))
        return rc;
    if (!mean_lum) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return LUMAHIP_OK;
    }
    float st[3];
    if ((rc = read_small(c, st, c->d_stats, 3, c->stream)))  // synchronises the stream
        return rc;
    *mean_lum = st[0] / (float)((int)w * (int)h);
    if (mean_needs_reference_sum(*mean_lum, st[1], w, h)) {
        if ((rc = ensure(c, (void **)&c->d_frame, &c->d_frame_cap, (size_t)w * h * sizeof(float))))
            return rc;
        if ((rc = transcode_channel0(c, src.dev(), src_sc, w, h, dst_sc, c->d_frame, c->stream)))
            return rc;
        return seq_mean(c, c->d_frame, w, h, mean_lum);
    }
    return LUMAHIP_OK;
}

// The same at half resolution (lumahip_transcode_half_frames_device): the destination set is staged and downloaded at (w/2) x (h/2).
// No mean_lum: the reference has no half-resolution operation whose sequential sum it could reproduce.
extern "C" int lumahip_transcode_half_frame_host(lumahip_ctx *c, const unsigned char *const src_planes[3], const int src_stride[3], int src_profile,
                                                 float src_sc, unsigned w, unsigned h, unsigned char *const dst_planes[3], const int dst_stride[3],
                                                 int dst_profile, float dst_sc)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!src_planes || !src_stride || !dst_planes || !dst_stride)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    StagedPlanes src{"source ", src_planes, src_stride, src_profile}, dst{"destination ", dst_planes, dst_stride, dst_profile};
    int rc = planes_staging(c, w, h, &src, &dst, true, 2);
    if (rc)
        return rc;
    if ((rc = planes_up(c, src, h)) ||
        (rc = transcode_half_impl(c, src.dev(), src_sc, 1, w, h, {dst.dp, dst_stride, NO_PFS, dst_profile}, dst_sc, nullptr, {c->stream, false})) ||
        (rc = planes_d2h(c, dst_planes, dst.dp, dst_stride, dst.L, 0, h / 2, c->stream, false)))
        return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LUMAHIP_OK;
}

// The same at quarter resolution (lumahip_transcode_quarter_frames_device, include/lumahip_rungs.h): the destination set is staged and
// downloaded at (w/4) x (h/4).  No mean_lum, as above.
extern "C" int lumahip_transcode_quarter_frame_host(lumahip_ctx *c, const unsigned char *const src_planes[3], const int src_stride[3], int src_profile,
                                                    float src_sc, unsigned w, unsigned h, unsigned char *const dst_planes[3], const int dst_stride[3],
                                                    int dst_profile, float dst_sc)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!src_planes || !src_stride || !dst_planes || !dst_stride)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    StagedPlanes src{"source ", src_planes, src_stride, src_profile}, dst{"destination ", dst_planes, dst_stride, dst_profile};
    int rc = planes_staging(c, w, h, &src, &dst, true, 4);
    if (rc)
        return rc;
    if ((rc = planes_up(c, src, h)) ||
        (rc = transcode_quarter_impl(c, src.dev(), src_sc, 1, w, h, {dst.dp, dst_stride, NO_PFS, dst_profile}, dst_sc, nullptr, {c->stream, false})) ||
        (rc = planes_d2h(c, dst_planes, dst.dp, dst_stride, dst.L, 0, h / 4, c->stream, false)))
        return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LUMAHIP_OK;
}

// The one host form of the thirteen measuring _frame_host entry points: one frame's inputs in host memory -> what the call delivers
// (m, of one frame), synchronously on the context's stream.  The inputs: a float frame (frame; rgb may then not be null) and / or the
// plane sets src and tgt as planes_staging takes them (quantizers: its flag), which the context's staging holds while `dispatch(f, d_out,
// launch)` runs the family's device dispatch on them: f = the staged frame, d_out = m.words() device words.  scale: the light level's,
// or nullptr.  The errors come in one order for every call: null arguments, the block, the scale, the staging's (geometry, profiles,
// quantizers, strides), out_words below a map's words (per-frame words: ignored) -- before anything is uploaded.
template <typename F>
static int measure_host(lumahip_ctx *c, const MeasureOut &m, bool frame, const float *rgb, StagedPlanes *src, StagedPlanes *tgt, bool quantizers,
                        const float *scale, uint64_t *out, size_t out_words, F dispatch, const SourceSize *full = nullptr)
{
    // full: the half-resolution calls -- the source set is staged at its own size, the set `tgt` at the record's, half of it
    const unsigned sw = full ? full->w : m.w, sh = full ? full->h : m.h;
    if (!c)
        return LUMAHIP_ERR_ARG;
    if ((frame && !rgb) || (src && (!src->planes || !src->stride)) || (tgt && (!tgt->planes || !tgt->stride)) || !out)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    int rc;
    // (the scale's test sits where it always sat: behind the size of a frame that comes alone, in front of a plane set's staging)
    if ((rc = m.check_block(c)) || (scale && ((!tgt && (rc = check_size(c, m.w, m.h))) || (rc = check_light_scale(c, *scale)))) ||
        (rc = planes_staging(c, sw, sh, src, tgt, quantizers, full ? full->scale : 1)))
        return rc;
    // (the words' count needs a checked geometry)
    if (m.map() && out_words < m.words())
        return fail(c, LUMAHIP_ERR_ARG, "%s: %zu words for a map of %zu", m.call, out_words, m.words());
    const size_t nfl = (size_t)3 * m.w * m.h;
    if ((rc = ensure(c, (void **)&c->d_arr, &c->d_arr_cap, m.bytes())) ||
        (frame && ((rc = ensure(c, (void **)&c->d_frame, &c->d_frame_cap, nfl * sizeof(float))) ||
                   (rc = xfer_h2d(c, c->d_frame, rgb, nfl * sizeof(float), c->stream)))) ||
        (src && (rc = planes_up(c, *src, sh))) || (tgt && (rc = planes_up(c, *tgt, m.h))) ||
        (rc = dispatch(packed_frames(static_cast<const float *>(c->d_frame), nfl, 1, m.w, m.h), reinterpret_cast<uint64_t *>(c->d_arr),
                       StreamLaunch{c->stream, false})))
        return rc;
    return words_down(c, out, m.words());
}

// ... of the frame-fed calls (lumahip_distortion.hip): one float frame and given planes
static int measure_frame_host(lumahip_ctx *c, const float *rgb, float sc, int profile, const unsigned char *const planes[3], const int stride[3],
                              const MeasureOut &m, uint64_t *out, size_t out_words)
{
    StagedPlanes given{"", planes, stride, profile};
    return measure_host(c, m, true, rgb, nullptr, &given, true, nullptr, out, out_words, [&](const SrcFrames &f, uint64_t *d, const StreamLaunch &o) {
        return measure_frames_impl(c, f, sc, given.dev(), m, d, o);
    });
}

// ... of the plane-fed calls (lumahip_transcode.hip): source planes and given planes
static int measure_planes_host(lumahip_ctx *c, const unsigned char *const src_planes[3], const int src_stride[3], int src_profile, float src_sc,
                               const unsigned char *const given_planes[3], const int given_stride[3], int dst_profile, float dst_sc,
                               const MeasureOut &m, uint64_t *out, size_t out_words, const SourceSize *full = nullptr)
{
    StagedPlanes src{"source ", src_planes, src_stride, src_profile}, given{"given ", given_planes, given_stride, dst_profile};
    return measure_host(
        c, m, false, nullptr, &src, &given, true, nullptr, out, out_words,
        [&](const SrcFrames &, uint64_t *d, const StreamLaunch &o) { return measure_planes_impl(c, src.dev(), src_sc, given.dev(), dst_sc, m, d, o, full); },
        full);
}

// ... of the plane-to-plane calls (lumahip_planes_measure.hip): two plane sets of one profile; no quantizer is read
static int compare_planes_host(lumahip_ctx *c, const unsigned char *const a_planes[3], const int a_stride[3], const unsigned char *const b_planes[3],
                               const int b_stride[3], int profile, const MeasureOut &m, uint64_t *out, size_t out_words)
{
    StagedPlanes a{"set A ", a_planes, a_stride, profile}, b{"set B ", b_planes, b_stride, profile};
    return measure_host(c, m, false, nullptr, &a, &b, false, nullptr, out, out_words, [&](const SrcFrames &, uint64_t *d, const StreamLaunch &o) {
        return planes_measure_impl(c, a.dev(), b.dev(), m, d, o);
    });
}

extern "C" int lumahip_distortion_frame_host(lumahip_ctx *c, const float *rgb, unsigned w, unsigned h, float sc, int profile,
                                             const unsigned char *const planes[3], const int stride[3], uint64_t out[12])
{
    return measure_frame_host(c, rgb, sc, profile, planes, stride, {DistWhat::Frame, "distortion", 0, 1, w, h}, out, 12);
}

extern "C" int lumahip_distortion_map_frame_host(lumahip_ctx *c, const float *rgb, unsigned w, unsigned h, float sc, int profile,
                                                 const unsigned char *const planes[3], const int stride[3], unsigned block, uint64_t *map,
                                                 size_t map_words)
{
    return measure_frame_host(c, rgb, sc, profile, planes, stride, {DistWhat::Map, "distortion map", block, 1, w, h}, map, map_words);
}

extern "C" int lumahip_moments_map_frame_host(lumahip_ctx *c, const float *rgb, unsigned w, unsigned h, float sc, int profile,
                                              const unsigned char *const planes[3], const int stride[3], unsigned block, uint64_t *mom,
                                              size_t mom_words)
{
    return measure_frame_host(c, rgb, sc, profile, planes, stride, {DistWhat::Moments, "moments map", block, 1, w, h}, mom, mom_words);
}

extern "C" int lumahip_transcode_distortion_frame_host(lumahip_ctx *c, const unsigned char *const src_planes[3], const int src_stride[3],
                                                       int src_profile, float src_sc, unsigned w, unsigned h,
                                                       const unsigned char *const given_planes[3], const int given_stride[3], int dst_profile,
                                                       float dst_sc, uint64_t out[12])
{
    return measure_planes_host(c, src_planes, src_stride, src_profile, src_sc, given_planes, given_stride, dst_profile, dst_sc,
                               {DistWhat::Frame, "transcode distortion", 0, 1, w, h}, out, 12);
}

extern "C" int lumahip_transcode_distortion_map_frame_host(lumahip_ctx *c, const unsigned char *const src_planes[3], const int src_stride[3],
                                                           int src_profile, float src_sc, unsigned w, unsigned h,
                                                           const unsigned char *const given_planes[3], const int given_stride[3],
                                                           int dst_profile, float dst_sc, unsigned block, uint64_t *map, size_t map_words)
{
    return measure_planes_host(c, src_planes, src_stride, src_profile, src_sc, given_planes, given_stride, dst_profile, dst_sc,
                               {DistWhat::Map, "transcode distortion map", block, 1, w, h}, map, map_words);
}

extern "C" int lumahip_transcode_moments_map_frame_host(lumahip_ctx *c, const unsigned char *const src_planes[3], const int src_stride[3],
                                                        int src_profile, float src_sc, unsigned w, unsigned h,
                                                        const unsigned char *const given_planes[3], const int given_stride[3],
                                                        int dst_profile, float dst_sc, unsigned block, uint64_t *mom, size_t mom_words)
{
    return measure_planes_host(c, src_planes, src_stride, src_profile, src_sc, given_planes, given_stride, dst_profile, dst_sc,
                               {DistWhat::Moments, "transcode moments map", block, 1, w, h}, mom, mom_words);
}

// The two half-resolution calls (include/lumahip_ladder.h): w x h is the source's size, the given set and the words are of (w/2) x (h/2)
extern "C" int lumahip_transcode_half_distortion_frame_host(lumahip_ctx *c, const unsigned char *const src_planes[3], const int src_stride[3],
                                                            int src_profile, float src_sc, unsigned w, unsigned h,
                                                            const unsigned char *const given_planes[3], const int given_stride[3],
                                                            int dst_profile, float dst_sc, uint64_t out[12])
{
    const SourceSize full{w, h, 2};
    return measure_planes_host(c, src_planes, src_stride, src_profile, src_sc, given_planes, given_stride, dst_profile, dst_sc,
                               {DistWhat::Frame, "half-resolution transcode distortion", 0, 1, w / 2, h / 2}, out, 12, &full);
}

extern "C" int lumahip_transcode_half_distortion_map_frame_host(lumahip_ctx *c, const unsigned char *const src_planes[3], const int src_stride[3],
                                                                int src_profile, float src_sc, unsigned w, unsigned h,
                                                                const unsigned char *const given_planes[3], const int given_stride[3],
                                                                int dst_profile, float dst_sc, unsigned block, uint64_t *map, size_t map_words)
{
    const SourceSize full{w, h, 2};
    return measure_planes_host(c, src_planes, src_stride, src_profile, src_sc, given_planes, given_stride, dst_profile, dst_sc,
                               {DistWhat::Map, "half-resolution transcode distortion map", block, 1, w / 2, h / 2}, map, map_words, &full);
}

extern "C" int lumahip_planes_distortion_frame_host(lumahip_ctx *c, const unsigned char *const a_planes[3], const int a_stride[3], unsigned w,
                                                    unsigned h, const unsigned char *const b_planes[3], const int b_stride[3], int profile,
                                                    uint64_t out[12])
{
    return compare_planes_host(c, a_planes, a_stride, b_planes, b_stride, profile, {DistWhat::Frame, "planes distortion", 0, 1, w, h}, out, 12);
}

extern "C" int lumahip_planes_distortion_map_frame_host(lumahip_ctx *c, const unsigned char *const a_planes[3], const int a_stride[3],
                                                        unsigned w, unsigned h, const unsigned char *const b_planes[3], const int b_stride[3],
                                                        int profile, unsigned block, uint64_t *map, size_t map_words)
{
    return compare_planes_host(c, a_planes, a_stride, b_planes, b_stride, profile, {DistWhat::Map, "planes distortion map", block, 1, w, h}, map,
                               map_words);
}

extern "C" int lumahip_planes_moments_map_frame_host(lumahip_ctx *c, const unsigned char *const a_planes[3], const int a_stride[3],
                                                     unsigned w, unsigned h, const unsigned char *const b_planes[3], const int b_stride[3],
                                                     int profile, unsigned block, uint64_t *mom, size_t mom_words)
{
    return compare_planes_host(c, a_planes, a_stride, b_planes, b_stride, profile, {DistWhat::Moments, "planes moments map", block, 1, w, h}, mom,
                               mom_words);
}

// ---- content light level (lumahip_light_level.hip): one frame, or one frame's planes, up; one launch; the eight words down
extern "C" int lumahip_light_level_frame_host(lumahip_ctx *c, const float *rgb, unsigned w, unsigned h, float scale, uint64_t out[8])
{
    const MeasureOut m(DistWhat::Light, "light level", 0, 1, w, h);
    return measure_host(c, m, true, rgb, nullptr, nullptr, false, &scale, out, 0, [&](const SrcFrames &f, uint64_t *d, const StreamLaunch &o) {
        return light_level_impl(c, &f, nullptr, 1.0f, scale, m, d, o);
    });
}

extern "C" int lumahip_planes_light_level_frame_host(lumahip_ctx *c, const unsigned char *const planes[3], const int stride[3], unsigned w,
                                                     unsigned h, int profile, float sc, float scale, uint64_t out[8])
{
    const MeasureOut m(DistWhat::Light, "light level", 0, 1, w, h);
    StagedPlanes given{"", planes, stride, profile};   // (staged under the quantizer's demands: the geometry, the profile, its presence)
    return measure_host(c, m, false, nullptr, nullptr, &given, true, &scale, out, 0, [&](const SrcFrames &, uint64_t *d, const StreamLaunch &o) {
        const SrcPlanes pl = given.dev();
        return light_level_impl(c, nullptr, &pl, sc, scale, m, d, o);
    });
}

// ---- binary16 frames (halves by type): 6 B per pixel cross PCIe in either direction.  One piece, on the context's stream: the
// caller's halves go up as they are (no round-trip test, unlike the half upload above) and the decoded halves come down as the
// kernel wrote them.
extern "C" int lumahip_encode_frame_host_f16(lumahip_ctx *c, const uint16_t *rgb, unsigned w, unsigned h, float sc, int profile,
                                             unsigned char *const planes[3], const int stride[3], float *mean_lum)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    return encode_frame_host_impl(c, rgb, Elem::F16, w, h, sc, profile, planes, stride, mean_lum, nullptr, c->q.cs);
}

extern "C" int lumahip_decode_frame_host_f16(lumahip_ctx *c, const unsigned char *const planes[3], const int stride[3], unsigned w,
                                             unsigned h, int profile, float sc, uint16_t *rgb_out)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    return decode_frame_host_impl(c, planes, stride, w, h, profile, sc, rgb_out, Elem::F16, c->q.cs);
}

// ---- frames in the three device slots: the batched calls and the stream push / pop ---------------------------------------------
static int pipe_prepare(lumahip_ctx *c, size_t frame_bytes, size_t planes_bytes, unsigned nframes)
{
    if (int rc = pipe_streams(c))
        return rc;
    if (!c->slot[0].h2d) {
        for (auto &sl : c->slot) {
            HIPCHK(c, hipEventCreateWithFlags(&sl.h2d, hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&sl.kern, hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&sl.d2h, hipEventDisableTiming));
            HIPCHK(c, hipMalloc(&sl.d_stats, 3 * sizeof(float)));
        }
    }
    if (c->slot_frame_cap < frame_bytes || c->slot_planes_cap < planes_bytes) {
        HIPCHK(c, hipDeviceSynchronize());
        for (auto &sl : c->slot) {
            (void)hipFree(sl.d_frame);
            (void)hipFree(sl.d_planes);
            sl.d_frame = nullptr;
            sl.d_planes = nullptr;
            HIPCHK(c, hipMalloc(&sl.d_frame, frame_bytes));
            HIPCHK(c, hipMalloc(&sl.d_planes, planes_bytes));
        }
        c->slot_frame_cap = frame_bytes;
        c->slot_planes_cap = planes_bytes;
    }
    if (c->h_stats_cap < nframes) {
        if (c->h_stats)
            (void)hipHostFree(c->h_stats);
        c->h_stats = nullptr;
        HIPCHK(c, hipHostMalloc(&c->h_stats, (size_t)nframes * 3 * sizeof(float), hipHostMallocDefault));
        c->h_stats_cap = nframes;
    }
    return LUMAHIP_OK;
}

// What a slot stage does to one frame, in either direction; the batched loops and the pushes differ in where the frames come
// from and in what happens around the steps, not in the steps
namespace {
struct SlotFrame {
    lumahip_ctx *c;
    PlaneLayout L;
    const int *stride;
    unsigned w, h;
    int profile;
    float sc;
    size_t nfl() const { return (size_t)3 * w * h; }

    // encode: the caller's floats into the slot -- as halves (*as16) where the context wants to try and the frame holds halves,
    // with the half upload's bookkeeping; a frame that does not goes up as floats behind whatever part of it went up as halves
    // (same stream, same slot, nothing launched on it yet)
    int floats_up(lumahip_ctx::Slot &sl, const float *rgb, bool *as16) const
    {
        const bool try16 = in16_try(c, w, false);
        const int rc = upload_floats(c, {sl.d_frame, rgb, 0, nfl(), 1, 0}, c->s_h2d, try16, as16, [&] {
            in16_result(c, false);
            return (int)LUMAHIP_OK;
        });
        if (rc == LUMAHIP_OK && *as16)
            in16_result(c, true);
        return rc;
    }
    int encode(lumahip_ctx::Slot &sl, bool halves) const
    {
        unsigned char *dp[3];
        device_planes(dp, sl.d_planes, L, stride);
        const SrcFrames f = halves ? packed_frames<const uint16_t>(reinterpret_cast<const uint16_t *>(sl.d_frame), nfl(), 1, w, h)   // same element offsets
                                   : packed_frames<const float>(sl.d_frame, nfl(), 1, w, h);
        return encode_frames_device_impl(c, f, sc, {dp, stride, NO_PFS, profile}, sl.d_stats, {c->q.cs, c->s_kern, false, HalfSource::Upload});
    }
    int planes_down(lumahip_ctx::Slot &sl, unsigned char *const planes[3]) const
    {
        unsigned char *dp[3];
        device_planes(dp, sl.d_planes, L, stride);
        return planes_d2h(c, planes, dp, stride, L, 0, h, c->s_d2h, true);
    }
    // decode: the caller's planes into the slot.  all_pinned (the push asks): whether the copy engine reads every plane directly
    int planes_up(lumahip_ctx::Slot &sl, const unsigned char *const planes[3], bool *all_pinned = nullptr) const
    {
        unsigned char *dp[3];
        device_planes(dp, sl.d_planes, L, stride);
        int rc = LUMAHIP_OK;
        if (all_pinned)
            *all_pinned = true;
        for (int p = 0; p < 3 && rc == LUMAHIP_OK; p++) {
            if (all_pinned)
                *all_pinned = *all_pinned && host_range_is_pinned(planes[p], (size_t)(L.rows[p] - 1) * stride[p] + L.row_bytes[p]);
            rc = plane_h2d(c, dp, planes, stride, L, p, 0, h, c->s_h2d);
        }
        return rc;
    }
    int decode(lumahip_ctx::Slot &sl) const
    {
        unsigned char *dp[3];
        device_planes(dp, sl.d_planes, L, stride);
        return decode_impl(c, {dp, stride, NO_PFS, profile}, sc, packed_frames(sl.d_frame, nfl(), 1, w, h), {c->q.cs, c->s_kern});
    }
    int floats_down(lumahip_ctx::Slot &sl, float *rgb_out) const { return xfer_d2h_deferred(c, rgb_out, sl.d_frame, nfl() * sizeof(float), c->s_d2h); }
};
}  // namespace

// What the two batched calls open with: the arguments checked (frames[i]: frame i on the host, `what` names it), no pushed frame
// pending, the slots large enough.
template <typename T>
static int batch_begin(lumahip_ctx *c, T *const *frames, const char *what, const unsigned char *const *planes, const int stride[3], unsigned nframes,
                       unsigned w, unsigned h, int profile, float sc, SlotFrame &f)
{
    if (!c || !frames || !planes || !stride || nframes == 0)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    if (int rc = check_geom(c, w, h, profile, c->q.cs))
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    f = SlotFrame{c, {}, stride, w, h, profile, sc};
    plane_layout(f.L, w, h, profile, stride);
    for (unsigned i = 0; i < nframes; i++) {
        if (!frames[i])
            return fail(c, LUMAHIP_ERR_ARG, "null %s %u", what, i);
        const int p = bad_plane(f.L, planes + 3 * i, stride);
        if (p >= 0)
            return fail(c, LUMAHIP_ERR_ARG, "frame %u plane %d: null or stride too small", i, p);
    }
    if (c->es_head != c->es_tail)
        return fail(c, LUMAHIP_ERR_STATE, "frames pushed with lumahip_encode_stream_push / lumahip_decode_stream_push are still pending: pop them first");
    return pipe_prepare(c, f.nfl() * sizeof(float), f.L.total, nframes);
}

extern "C" int lumahip_encode_frames_host(lumahip_ctx *c, const float *const *rgb, unsigned nframes, unsigned w, unsigned h,
                                          float sc, int profile, unsigned char *const *planes, const int stride[3],
                                          float *mean_lum)
{
    SlotFrame f;
    int rc = batch_begin(c, rgb, "frame", planes, stride, nframes, w, h, profile, sc, f);
    if (rc)
        return rc;
    // Download chunks sized for these planes: the pipelined ENCODE paths only (this call and the encode push).  The decode
    // pipelines download floats with the default chunk.
    if ((rc = dn_chunks_for(c, f.L.total)))
        return rc;
    bool as16 = false;   // of the frame being issued
    rc = pipe_run(
        c, nframes, [&](unsigned i) { return slot_stage(c->slot[i % 3], i); },
        [&](unsigned i) { return f.floats_up(c->slot[i % 3], rgb[i], &as16); },
        [&](unsigned i, const PipeStage &) { return f.encode(c->slot[i % 3], as16); },
        [&](unsigned i) { return f.planes_down(c->slot[i % 3], planes + 3 * i); }, c->h_stats);
    if (rc == LUMAHIP_OK && mean_lum)
        for (unsigned i = 0; i < nframes && rc == LUMAHIP_OK; i++) {
            mean_lum[i] = c->h_stats[3 * (size_t)i] / (float)((int)w * (int)h);
            // rare: redo this frame's sum in the reference's order.  The slots have been reused by later frames, so the frame goes
            // up once more, into slot 0, on the context's stream (the pop of a pushed frame still finds it in its slot)
            if (mean_needs_reference_sum(mean_lum[i], c->h_stats[3 * (size_t)i + 1], w, h)) {
                if ((rc = xfer_h2d(c, c->slot[0].d_frame, rgb[i], f.nfl() * sizeof(float), c->stream)))
                    return rc;
                rc = mean_luminance_reference_impl(c, c->slot[0].d_frame, Elem::F32, w, h, sc, c->q.cs, &mean_lum[i]);
            }
        }
    return rc;
}

extern "C" int lumahip_decode_frames_host(lumahip_ctx *c, const unsigned char *const *planes, const int stride[3],
                                          unsigned nframes, unsigned w, unsigned h, int profile, float sc,
                                          float *const *rgb_out)
{
    SlotFrame f;
    if (int rc = batch_begin(c, rgb_out, "output frame", planes, stride, nframes, w, h, profile, sc, f))
        return rc;
    return pipe_run(
        c, nframes, [&](unsigned i) { return slot_stage(c->slot[i % 3], i); },
        [&](unsigned i) { return f.planes_up(c->slot[i % 3], planes + 3 * i); },
        [&](unsigned i, const PipeStage &) { return f.decode(c->slot[i % 3]); },
        [&](unsigned i) { return f.floats_down(c->slot[i % 3], rgb_out[i]); });
}

// ---- streaming form of the batched calls: frames arrive one at a time ---------------------------------------------------------
// lumahip_encode_frames_host needs the whole batch in hand.  A caller that gets its frames one by one (the reference's
// `for (...) encoder.encode(&frame)` loop, lumaenc.cpp:205-243) can still overlap the tail of frame i (kernel, download,
// copy out of the staging chunks) with the upload of frame i+1 by accepting ONE frame of latency: push(i+1), then pop(i).
// Same three device slots and three streams as the batched form; at most two frames in flight.  The decode counterpart
// (LumaDecoder::decode() in a loop, lumadec.cpp:112-160): the download of frame i (12 B/pixel, the heavy direction here) keeps
// the copy engine busy while the planes of frame i+1 go up and its kernel runs.
// The pipeline's loop is carried across the calls: a push is pipe_issue and pipe_fetch of the SAME frame, its download queued
// behind its kernel; the pop completes that download.
static const char *const PUSH_NAME[2] = {"lumahip_encode_stream_push", "lumahip_decode_stream_push"};
static const char *const POP_NAME[2] = {"lumahip_encode_stream_pop", "lumahip_decode_stream_pop"};

// What a push opens with (dir 0: encode, 1: decode; frame: the caller's colour frame): the arguments and the state of the
// stream checked, the slots large enough (reallocated only when nothing is in flight: same geometry otherwise)
static int push_begin(lumahip_ctx *c, int dir, const void *frame, const unsigned char *const planes[3], const int stride[3], unsigned w,
                      unsigned h, int profile, float sc, SlotFrame &f)
{
    if (!c || !frame || !planes || !stride)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    if (int rc = check_geom(c, w, h, profile, c->q.cs))
        return rc;
    const bool in_flight = c->es_head != c->es_tail;
    if (in_flight && c->es_dir != dir)
        return fail(c, LUMAHIP_ERR_STATE, "frames pushed with %s are in flight: pop them first", PUSH_NAME[1 - dir]);
    if (c->es_head - c->es_tail >= 2)
        return fail(c, LUMAHIP_ERR_STATE, "two frames are in flight already: %s the oldest first", POP_NAME[dir]);
    if (in_flight && (w != c->es_w || h != c->es_h || profile != c->es_profile || stride[0] != c->es_stride[0] ||
                      stride[1] != c->es_stride[1] || stride[2] != c->es_stride[2]))
        return fail(c, LUMAHIP_ERR_STATE, "frame geometry (size, profile or plane strides) changed while a frame is in flight: pop it first");
    HIPCHK(c, hipSetDevice(c->device));
    f = SlotFrame{c, {}, stride, w, h, profile, sc};
    plane_layout(f.L, w, h, profile, stride);
    if (const int p = bad_plane(f.L, planes, stride); p >= 0)
        return fail(c, LUMAHIP_ERR_ARG, "plane %d: null or stride too small", p);
    return pipe_prepare(c, f.nfl() * sizeof(float), f.L.total, 1);
}

// The frame with the next sequence number through its slot.  upload(slot, &pinned_in) also says whether the copy engine reads
// the caller's memory directly; h_stats as in pipe_fetch.
template <typename Upload, typename Launch, typename Download>
static int push_frame(const SlotFrame &f, int dir, Upload upload, Launch launch, Download download, float *h_stats)
{
    lumahip_ctx *const c = f.c;
    const unsigned seq = c->es_head;
    lumahip_ctx::Slot &sl = c->slot[seq % 3];
    const PipeStage st = slot_stage(sl, seq);
    c->up_ramp = 0;   // (per push, as per single-frame call)
    // Until the frame counts as pushed, a failure drops the download chunks queued for it: they carry the tag seq + 1 (0: the
    // chunks of the plain calls), which is set only while this frame's downloads are queued
    DnGuard guard{c, false, seq + 1};
    bool pinned_in = false;
    int rc = pipe_issue(c, st, [&] { return upload(sl, &pinned_in); }, [&] { return launch(sl); });
    if (rc)
        return rc;
    // the output comes down behind the kernel; pageable destinations are emptied out of the staging chunks by the pop (or
    // earlier, when the ring comes round)
    rc = pipe_fetch(c, st, [&] {
        c->d2h_tag = seq + 1;
        const int r = download(sl);
        c->d2h_tag = 0;
        return r;
    }, h_stats);
    if (rc)
        return rc;
    // The copy engine read the caller's pinned memory directly: it must be done with it when the push returns.  (The batched
    // forms rely on the stream syncs of their drain instead.)
    if (pinned_in)
        HIPCHK(c, hipEventSynchronize(st.h2d));
    c->es_w = f.w;
    c->es_h = f.h;
    c->es_profile = f.profile;
    c->es_sc = f.sc;
    for (int p = 0; p < 3; p++)
        c->es_stride[p] = f.stride[p];
    c->es_dir = dir;
    c->es_head = seq + 1;
    guard.armed = false;   // the pop completes them
    return LUMAHIP_OK;
}

// the oldest pushed frame: its download chunks copied out, its slot's downloads done.  *seq: its sequence number
static int pop_frame(lumahip_ctx *c, int dir, unsigned *seq)
{
    if (c->es_head == c->es_tail || c->es_dir != dir)
        return fail(c, LUMAHIP_ERR_STATE, dir ? "no decode frame is in flight" : "no encode frame is in flight");
    HIPCHK(c, hipSetDevice(c->device));
    *seq = c->es_tail;
    c->es_tail = *seq + 1;                        // (popped even if something below fails: nothing may stay half-finished)
    const int rc = d2h_flush(c, seq);
    HIPCHK(c, hipEventSynchronize(c->slot[*seq % 3].d2h));      // downloads into pinned memory (no chunks to flush), and the statistics
    return rc;
}

extern "C" int lumahip_encode_stream_push(lumahip_ctx *c, const float *rgb, unsigned w, unsigned h, float sc, int profile,
                                          unsigned char *const planes[3], const int stride[3])
{
    SlotFrame f;
    int rc = push_begin(c, 0, rgb, planes, stride, w, h, profile, sc, f);
    if (rc)
        return rc;
    // download chunks sized for these planes, as in lumahip_encode_frames_host; they can only be re-allocated while nothing is in flight
    if (c->es_head == c->es_tail && (rc = dn_chunks_for(c, f.L.total)))
        return rc;
    if (!c->h_es_stats)
        HIPCHK(c, hipHostMalloc((void **)&c->h_es_stats, 3 * 3 * sizeof(float), hipHostMallocDefault));
    const unsigned slot = c->es_head % 3;
    return push_frame(
        f, 0,
        [&](lumahip_ctx::Slot &sl, bool *pinned_in) {
            *pinned_in = host_range_is_pinned(rgb, f.nfl() * sizeof(float));
            bool as16 = false;
            if (int r = f.floats_up(sl, rgb, &as16))
                return r;
            if (as16)   // half upload: the CPU converted out of the caller's memory (pinned or not), so it is free again already
                *pinned_in = false;
            c->slot_in16[slot] = as16;
            return (int)LUMAHIP_OK;
        },
        [&](lumahip_ctx::Slot &sl) { return f.encode(sl, c->slot_in16[slot]); },
        [&](lumahip_ctx::Slot &sl) { return f.planes_down(sl, planes); }, c->h_es_stats + 3 * slot);
}

extern "C" int lumahip_encode_stream_pop(lumahip_ctx *c, float *mean_lum)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    unsigned seq;
    if (int rc = pop_frame(c, 0, &seq))
        return rc;
    if (mean_lum) {
        const float *stp = c->h_es_stats + 3 * (seq % 3);
        *mean_lum = stp[0] / (float)((int)c->es_w * (int)c->es_h);
        if (mean_needs_reference_sum(*mean_lum, stp[1], c->es_w, c->es_h))   // the slot still holds the frame as it was uploaded
            return mean_luminance_reference_impl(c, c->slot[seq % 3].d_frame, c->slot_in16[seq % 3] ? Elem::F16 : Elem::F32, c->es_w, c->es_h, c->es_sc, c->q.cs, mean_lum);
    }
    return LUMAHIP_OK;
}

extern "C" int lumahip_encode_stream_pending(const lumahip_ctx *c) { return (c && c->es_dir == 0) ? (int)(c->es_head - c->es_tail) : 0; }

extern "C" int lumahip_decode_stream_push(lumahip_ctx *c, const unsigned char *const planes[3], const int stride[3], unsigned w,
                                          unsigned h, int profile, float sc, float *rgb_out)
{
    SlotFrame f;
    if (int rc = push_begin(c, 1, rgb_out, planes, stride, w, h, profile, sc, f))
        return rc;
    return push_frame(
        f, 1, [&](lumahip_ctx::Slot &sl, bool *pinned_in) { return f.planes_up(sl, planes, pinned_in); },
        [&](lumahip_ctx::Slot &sl) { return f.decode(sl); }, [&](lumahip_ctx::Slot &sl) { return f.floats_down(sl, rgb_out); }, nullptr);
}

extern "C" int lumahip_decode_stream_pop(lumahip_ctx *c)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    unsigned seq;
    return pop_frame(c, 1, &seq);
}

extern "C" int lumahip_decode_stream_pending(const lumahip_ctx *c) { return (c && c->es_dir == 1) ? (int)(c->es_head - c->es_tail) : 0; }

extern "C" int lumahip_transform_color_space_host(lumahip_ctx *c, float *frame, unsigned w, unsigned h, int toCs, float sc)
{
    if (!c || !frame)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    if (!c->have_quant)
        return fail(c, LUMAHIP_ERR_STATE, "quantizer not set");
    if (c->q.cs < 0 || c->q.cs > 3)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "Error! Unrecognized color transformation");
    if (w == 0 || h == 0)
        return LUMAHIP_OK;  // the reference loops zero times and returns true
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)w * h, nfl = 3 * n;
    // device copy padded to an even pixel count per channel so the pair kernel applies to odd sizes too
    const size_t npad = (n + 1) & ~(size_t)1;
    int rc = ensure(c, (void **)&c->d_frame, &c->d_frame_cap, 3 * npad * sizeof(float));
    if (rc)
        return rc;
    if (npad == n) {
        if ((rc = xfer_h2d(c, c->d_frame, frame, nfl * sizeof(float), c->stream)))
            return rc;
    } else {
        HIPCHK(c, hipMemsetAsync(c->d_frame, 0, 3 * npad * sizeof(float), c->stream));
        for (int ch = 0; ch < 3; ch++)
            if ((rc = xfer_h2d(c, c->d_frame + ch * npad, frame + ch * n, n * sizeof(float), c->stream)))
                return rc;
    }
    // the kernel addresses channels at chan_stride = (w*h); present the padded buffer as a (npad x 1) frame
    rc = lumahip_transform_color_space_device(c, c->d_frame, 3 * npad, 1, (unsigned)npad, 1, toCs, sc);
    if (rc)
        return rc;
    if (npad == n) {
        if ((rc = xfer_d2h(c, frame, c->d_frame, nfl * sizeof(float), c->stream)))
            return rc;
    } else {
        for (int ch = 0; ch < 3; ch++)
            if ((rc = xfer_d2h(c, frame + ch * n, c->d_frame + ch * npad, n * sizeof(float), c->stream)))
                return rc;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LUMAHIP_OK;
}

static int array_op(lumahip_ctx *c, const float *in, float *out, size_t n, unsigned ch, bool quant)
{
    if (!c || !in || !out)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    if (!c->have_quant)
        return fail(c, LUMAHIP_ERR_STATE, "quantizer not set");
    if (n == 0)
        return LUMAHIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure(c, (void **)&c->d_arr, &c->d_arr_cap, 2 * n * sizeof(float));
    if (rc)
        return rc;
    if ((rc = xfer_h2d(c, c->d_arr, in, n * sizeof(float), c->stream)))
        return rc;
    if ((rc = array_launch(c, c->d_arr, c->d_arr + n, n, ch, quant)))
        return rc;
    if ((rc = xfer_d2h(c, out, c->d_arr + n, n * sizeof(float), c->stream)))
        return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LUMAHIP_OK;
}

extern "C" int lumahip_quantize_array_host(lumahip_ctx *c, const float *in, float *out, size_t n, unsigned ch)
{
    return array_op(c, in, out, n, ch, true);
}

extern "C" int lumahip_dequantize_array_host(lumahip_ctx *c, const float *in, float *out, size_t n, unsigned ch)
{
    return array_op(c, in, out, n, ch, false);
}

// LumaEncoder::setChannels / LumaDecoder::getVpxChannels on their own: no colour transform.  Channel 0
// goes through the LUT; channels 1,2 through the LUT for RGB / XYZ (src/luma_quantizer.cpp:219,251) --
// which is the CS_RGB kernel with sc = 1 (x*1.0f and x/1.0f are exact) -- and through the colour quantizer
// otherwise (CS_PACK).
static int pack_cs(const lumahip_ctx *c) { return (c->q.cs == CS_RGB || c->q.cs == CS_XYZ) ? CS_RGB : CS_PACK; }

extern "C" int lumahip_pack_frame_host(lumahip_ctx *c, const float *transformed, unsigned w, unsigned h, int profile,
                                       unsigned char *const planes[3], const int stride[3], float *mean_lum)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!c->have_quant)
        return fail(c, LUMAHIP_ERR_STATE, "quantizer not set");
    return encode_frame_host_impl(c, transformed, Elem::F32, w, h, 1.0f, profile, planes, stride, mean_lum, nullptr, pack_cs(c));
}

extern "C" int lumahip_unpack_frame_host(lumahip_ctx *c, const unsigned char *const planes[3], const int stride[3],
                                         unsigned w, unsigned h, int profile, float *dequantized_out)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!c->have_quant)
        return fail(c, LUMAHIP_ERR_STATE, "quantizer not set");
    return decode_frame_host_impl(c, planes, stride, w, h, profile, 1.0f, dequantized_out, Elem::F32, pack_cs(c));
}

