// Host-buffer half of the C ABI (include/apap_hip.h): error reporting, device
// selection, a small grow-only pool of device buffers, and the synchronous entry
// points that copy caller-owned numpy-style buffers to the GPU, enqueue the kernels
// through the "_device" entry points and copy the results back.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "apap_internal.h"

namespace {

thread_local char g_err[512] = "";

using namespace apap;   // DevSlot, S_* slot names

// The device buffers that host-buffer calls reuse live in the caller's context.  Calls made with
// a NULL context share this one pool (a cache: no option or result depends on it) and are
// serialised on its mutex - the reference is single-threaded, ctypes releases the GIL, so guard.
apap_ctx g_shared;

int slot_get(apap_ctx *pool, int which, size_t bytes, int dev, void **out) {
    DevSlot &s = pool->slots[which];
    if (bytes == 0) bytes = 4;
    if (s.ptr && (s.cap < bytes || s.dev != dev)) {
        (void)hipFree(s.ptr);
        s.ptr = nullptr;
        s.cap = 0;
    }
    if (!s.ptr) {
        // +16: the warp gather reads one dword at a 3-byte pixel and may touch 1 byte
        // past the image; keep that inside the allocation for pooled buffers.
        const hipError_t e = hipMalloc(&s.ptr, bytes + 16);
        if (e != hipSuccess) return apap::hip_fail((int)e, "hipMalloc of a pooled buffer");
        s.cap = bytes;
        s.dev = dev;
    }
    *out = s.ptr;
    return APAP_OK;
}

int select_device(int device, int *chosen) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count < 1) {
        (void)hipGetLastError();
        return apap::fail(APAP_ERR_NO_DEVICE,
                          "no HIP device visible (%s); this engine has no CPU fallback",
                          e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    }
    if (device >= count) return apap::fail(APAP_ERR_NO_DEVICE, "device %d requested, %d visible", device, count);
    if (device >= 0) {
        if ((e = hipSetDevice(device)) != hipSuccess) return apap::hip_fail((int)e, "hipSetDevice");
        *chosen = device;
    } else {
        if ((e = hipGetDevice(chosen)) != hipSuccess) return apap::hip_fail((int)e, "hipGetDevice");
    }
    return APAP_OK;
}

// Bytes [at, at + bytes) of a pooled buffer.  The address is read from the slot when the part is used, so a part may
// be taken before its slot is allocated.
struct Part {
    void *const *base;
    size_t at, bytes;
    template <class T>
    T *as() const { return (T *)((char *)*base + at); }
    Part first(size_t n) const { return Part{base, at, n}; }   // its leading n bytes
};

// The parts of one pooled buffer, each on a 256-byte boundary.  A part may be empty (an output the caller did not ask
// for): it keeps its place in the order and takes no room.
struct Layout {
    int which;
    void *const *base;
    size_t total = 0;
    Part take(size_t bytes) {
        const Part p{base, total, bytes};
        total += up256(bytes);
        return p;
    }
};

// One synchronous host-buffer call.  It holds the pool's lock and the selected device, hands out the pooled slots and
// enqueues copies on the null stream.  The first failure is kept: every later slot, copy and wait() does nothing and
// rc() returns it, so a call checks rc() once before it launches and returns wait() at its end.
// Whatever way the call is left, the stream is drained before the lock is released (the body of the destructor runs
// before the members go): no copy into or out of host memory outlives the call, and the next holder of the pool finds
// its buffers idle.  Host buffers of the call's own that a copy reads or writes (std::vector, stack variables) are
// declared BEFORE the HostCall, so that they die after it.
class HostCall {
  public:
    explicit HostCall(apap_ctx *ctx) : pool_(ctx ? ctx : &g_shared), lock_(pool_->mu) {}
    ~HostCall() {
        if (busy_) (void)hipStreamSynchronize(nullptr);
    }
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;

    int select(int device) { return rc_ = select_device(device, &dev_); }
    apap_ctx *pool() const { return pool_; }
    int dev() const { return dev_; }
    int rc() const { return rc_; }

    Part slot(int which, size_t bytes) {
        void *p;
        if (!rc_) rc_ = slot_get(pool_, which, bytes, dev_, &p);
        return Part{&pool_->slots[which].ptr, 0, bytes};
    }
    Layout layout(int which) const { return Layout{which, &pool_->slots[which].ptr}; }
    void alloc(const Layout &l) { (void)slot(l.which, l.total); }

    void up(const Part &to, const void *host) {
        if (!rc_) check(hipMemcpyAsync(to.as<void>(), host, to.bytes, hipMemcpyHostToDevice, (hipStream_t)stream()), "host-buffer call: upload");
    }
    void down(void *host, const Part &from) {
        if (!rc_) check(hipMemcpyAsync(host, from.as<void>(), from.bytes, hipMemcpyDeviceToHost, (hipStream_t)stream()), "host-buffer call: download");
    }
    void zero(const Part &p) {
        if (!rc_) check(hipMemsetAsync(p.as<void>(), 0, p.bytes, (hipStream_t)stream()), "host-buffer call: zero fill");
    }
    // The stream of the call, for the "_device" entry points: the null stream.  Whoever asks for it enqueues on it, and
    // the drain relies on the converse: nothing in a host-buffer call passes a literal nullptr as a stream, or enqueues
    // on the null stream in any other way than through this object.
    void *stream() {
        busy_ = true;
        return nullptr;
    }
    int wait() {
        if (rc_) return rc_;
        check(hipStreamSynchronize(nullptr), "host-buffer call: synchronize");
        if (!rc_) busy_ = false;
        return rc_;
    }

  private:
    void check(hipError_t e, const char *what) {
        if (e != hipSuccess) rc_ = apap::hip_fail((int)e, what);
    }
    apap_ctx *pool_;
    std::unique_lock<std::mutex> lock_;
    int dev_ = -1, rc_ = APAP_OK;
    bool busy_ = false;   // something was enqueued on the null stream since the last completed wait()
};

// offset[0 .. count] relative to offset[0]: the device arrays of a batch start at its first pair or image
std::vector<int> relative_offsets(const int *offset, int count) {
    std::vector<int> rel((size_t)count + 1);
    for (int p = 0; p <= count; ++p) rel[p] = offset[p] - offset[0];
    return rel;
}

// The images of a batch side by side in S_IMG: their parts, the slot allocated ...
std::vector<Part> image_parts(HostCall &call, const int *heights, const int *widths, const int *channels, int n_images) {
    Layout lay = call.layout(S_IMG);
    std::vector<Part> parts((size_t)n_images, Part{});
    for (int m = 0; m < n_images; ++m) parts[m] = lay.take((size_t)heights[m] * widths[m] * channels[m]);
    call.alloc(lay);
    return parts;
}
// ... and one upload each; returns their device addresses.
std::vector<const uint8_t *> upload_images(HostCall &call, const std::vector<Part> &parts, const uint8_t *const *imgs) {
    std::vector<const uint8_t *> d_imgs(parts.size(), nullptr);
    for (size_t m = 0; m < parts.size() && !call.rc(); ++m) {
        d_imgs[m] = parts[m].as<const uint8_t>();
        call.up(parts[m], imgs[m]);
    }
    return d_imgs;
}

// The distinct host pictures of a call, uploaded once each: problems and layers may share a picture (the reference's
// baseline / result pair), told by its address and size.  Declared before the HostCall, like every host vector of a call.
struct Pictures {
    struct Pic { const uint8_t *host; size_t bytes; Part dev; };
    std::vector<Pic> pics;   // in the order of their first add(): the order of their parts and uploads
    std::map<std::pair<const uint8_t *, size_t>, int> seen;
    // The index of the picture.  `shared` false: a picture of its own, whatever was added before or comes after.
    int add(const uint8_t *host, size_t bytes, bool shared = true) {
        const int next = (int)pics.size();
        if (shared) {
            const auto it = seen.emplace(std::make_pair(host, bytes), next);
            if (!it.second) return it.first->second;
        }
        pics.push_back(Pic{host, bytes, Part{}});
        return next;
    }
    void take(Layout &lay) { for (Pic &p : pics) p.dev = lay.take(p.bytes); }
    void upload(HostCall &call) const { for (const Pic &p : pics) call.up(p.dev, p.host); }
    const uint8_t *dev(int k) const { return pics[k].dev.as<const uint8_t>(); }
};

int status_to_code(int status, const char *who) {
    if (status & APAP_STATUS_SINGULAR) return apap::fail(APAP_ERR_SINGULAR, "%s: Singular matrix", who);
    if (status & APAP_STATUS_INDEX)
        return apap::fail(APAP_ERR_INDEX, "%s: index 0 is out of bounds for axis 0 with size 0 (mesh edges do not cover the canvas)", who);
    if (status & APAP_STATUS_UNPREPARED)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: the warp workspace holds no lookup tables for this mesh / canvas (APAP_WARP_GEOMETRY)", who);
    return APAP_OK;
}

}  // namespace

namespace apap {
int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace apap

extern "C" {

const char *apap_last_error(void) { return g_err; }
const char *apap_version(void) { return "cvx_proj_amd apap-hip " APAP_ABI_VERSION_STRING " (gfx950)"; }
int apap_abi_version(void) { return APAP_ABI_VERSION; }

int apap_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return count;
}

// The weight tensor of `cells` cells, streamed through a bounded device buffer (it is 8 n bytes per cell):
// `table` / `vert` are resident, W_out is the host destination.  1 GiB of device staging by default;
// APAP_OPT_WEIGHT_CHUNK_KB lets tests force several chunks.
static int stream_weights(apap_ctx *ctx, HostCall &call, const Part &table, int n, const Part &vert, int cells, double gamma,
                          double sigma, double *W_out) {
    const size_t max_bytes = (size_t)apap::opt(ctx, APAP_OPT_WEIGHT_CHUNK_KB) << 10;
    int chunk = (int)(max_bytes / ((size_t)n * sizeof(double)));
    if (chunk < 1) chunk = 1;
    if (chunk > cells) chunk = cells;
    const Part W = call.slot(S_W, (size_t)chunk * n * sizeof(double));
    int rc = call.rc();
    for (int c0 = 0; !rc && c0 < cells; c0 += chunk) {
        const int nc = cells - c0 < chunk ? cells - c0 : chunk;
        rc = apap_weights_device(ctx, table.as<const double>(), n, vert.as<const double>() + (size_t)2 * c0, nc, gamma, sigma,
                                 W.as<double>(), call.stream());
        if (rc) return rc;
        call.down(W_out + (size_t)c0 * n, W.first((size_t)nc * n * sizeof(double)));
        rc = call.wait();
    }
    return rc;
}

int apap_local_weights(apap_ctx *ctx, const float *src, int n, const double *vertices, int cells, double gamma,
                       double sigma, double *W_out, int device) {
    return apap_local_weights_pts(ctx, src, 0, n, vertices, cells, gamma, sigma, W_out, device);
}

int apap_local_weights_pts(apap_ctx *ctx, const void *src, int src_f64, int n, const double *vertices, int cells, double gamma,
                           double sigma, double *W_out, int device) {
    if (!src || !vertices || !W_out) return apap::fail(APAP_ERR_INVALID_ARG, "apap_local_weights: null argument");
    if (n < 1 || cells < 1) return apap::fail(APAP_ERR_INVALID_ARG, "apap_local_weights: n=%d cells=%d", n, cells);
    std::vector<double> host_table;   // an upload reads it
    HostCall call(ctx);
    int rc = call.select(device);
    if (rc) return rc;
    // the weight kernel reads a keypoint's (x, y) from columns 30, 31 of its table row
    host_table.assign((size_t)n * APAP_TABLE_STRIDE, 0.0);
    for (int k = 0; k < n; ++k) {
        host_table[(size_t)k * APAP_TABLE_STRIDE + 30] = src_f64 ? ((const double *)src)[2 * k] : (double)((const float *)src)[2 * k];
        host_table[(size_t)k * APAP_TABLE_STRIDE + 31] = src_f64 ? ((const double *)src)[2 * k + 1] : (double)((const float *)src)[2 * k + 1];
    }
    const Part table = call.slot(S_TABLE, host_table.size() * sizeof(double));
    const Part vert = call.slot(S_VERT, (size_t)cells * 2 * sizeof(double));
    call.up(table, host_table.data());
    call.up(vert, vertices);
    return stream_weights(ctx, call, table, n, vert, cells, gamma, sigma, W_out);
}

int apap_local_homography(apap_ctx *ctx, const float *src, const float *dst, int n, const double *vertices,
                          int mesh_rows, int mesh_cols, double gamma, double sigma, float *H_out,
                          double *W_out, int device) {
    return apap_local_homography_pts(ctx, src, 0, dst, 0, n, vertices, mesh_rows, mesh_cols, gamma, sigma, H_out, W_out, device);
}

int apap_local_homography_pts(apap_ctx *ctx, const void *src, int src_f64, const void *dst, int dst_f64, int n,
                              const double *vertices, int mesh_rows, int mesh_cols, double gamma, double sigma, float *H_out,
                              double *W_out, int device) {
    if (!src || !dst || !vertices || !H_out) return apap::fail(APAP_ERR_INVALID_ARG, "apap_local_homography: null argument");
    if (n < 2 || mesh_rows < 1 || mesh_cols < 1)
        return apap::fail(APAP_ERR_INVALID_ARG, "apap_local_homography: n=%d mesh=%dx%d", n, mesh_rows, mesh_cols);
    if ((long long)mesh_rows * mesh_cols > (1ll << 30)) return apap::fail(APAP_ERR_INVALID_ARG, "apap_local_homography: mesh too large");
    std::vector<double> host_table;   // uploads read these two
    double host_denorm[APAP_DENORM_DOUBLES];
    HostCall call(ctx);
    int rc = call.select(device);
    if (rc) return rc;

    // once-per-pair set-up on the host (apap.py:132-145)
    // in the dtype of each keypoint set, as the reference's own functions run (float64 keypoints stay float64 up to the
    // float32 rounding of the matrices and of the DLT rows)
    float N1[9], N2[9], C1[9], C2[9], iC2[9], iN2[9];
    std::vector<double> cf1((size_t)2 * n), cf2((size_t)2 * n), src64((size_t)2 * n);
    std::vector<float> aa((size_t)18 * n);
    rc = apap_host_prepare_pts(src, src_f64, dst, dst_f64, n, N1, N2, C1, C2, iC2, iN2, nullptr, nullptr, cf1.data(), cf2.data());
    if (rc) return rc;
    if ((rc = apap_host_dlt_rows_pts(cf1.data(), cf2.data(), n, src_f64 || dst_f64, aa.data()))) return rc;
    for (size_t i = 0; i < (size_t)2 * n; ++i) src64[i] = src_f64 ? ((const double *)src)[i] : (double)((const float *)src)[i];
    host_table.resize((size_t)n * APAP_TABLE_STRIDE);
    rc = apap::opt(ctx, APAP_OPT_MOMENTS) == 24 ? apap_host_build_table24(src64.data(), aa.data(), n, host_table.data())
                                                : apap_host_build_table_rows(src64.data(), aa.data(), n, host_table.data());
    if (rc) return rc;
    if ((rc = apap_host_build_denorm(iC2, C1, iN2, N1, host_denorm))) return rc;

    const int cells = mesh_rows * mesh_cols;
    const Part table = call.slot(S_TABLE, host_table.size() * sizeof(double));
    const Part vert = call.slot(S_VERT, (size_t)cells * 2 * sizeof(double));
    const Part denorm = call.slot(S_DENORM, sizeof(host_denorm));
    const Part H = call.slot(S_H, (size_t)cells * 9 * sizeof(float));
    const Part work = call.slot(S_WORK, apap_solve_workspace_bytes(ctx, n, cells));
    call.up(table, host_table.data());
    call.up(vert, vertices);
    call.up(denorm, host_denorm);
    if ((rc = call.rc())) return rc;
    rc = apap_solve_device(ctx, table.as<const double>(), n, vert.as<const double>(), cells, gamma, sigma, denorm.as<const double>(),
                           H.as<float>(), work.as<void>(), work.bytes, call.stream());
    if (rc) return rc;
    call.down(H_out, H);
    if (W_out && (rc = stream_weights(ctx, call, table, n, vert, cells, gamma, sigma, W_out))) return rc;
    return call.wait();
}

// ---- apap_local_warp / apap_local_stitch with PCIe overlapped ---------------------------------------
// The call moves 25 MB up and 27 MB down around a 20 us kernel (4K pair): one after the other that is
// ~1.1 ms, almost all of it PCIe one way at a time.  Here the caller's buffers are pinned for the call, the
// source image goes up in row chunks on one stream, the canvas is warped in row bands on a second - band b
// as soon as the source rows it can read have landed - and every finished band goes down on a third while
// later chunks are still going up.  Measured on the MI355X boxes of this pool (a build with host and event time stamps - git tag r05-hooks -, 4K pair):
// 0.93 ms against 1.14 ms - the two directions do NOT add up here: 25 MB up alone and 27 MB down alone each move
// at ~56 GB/s, both together at ~60 GB/s in all (the same with the canvas written straight into the pinned host
// buffer by the kernel instead of a DMA copy), so what the overlap hides is the kernels, the set-up and the
// per-copy latencies, not half of the bytes.  And pinning is not free: the FIRST call on a buffer (a new virtual range)
// spends ~1 ms registering it and ~7 ms at its first DMA use; only later calls on the same buffers run at 0.93 ms
// (profiles/r03_pcie_overlap.txt).  Hence opt-in (APAP_OPT_OVERLAP_PCIE = 1): right for a caller that streams pairs through buffers it
// keeps, wrong for one warp into a fresh array - the default stays the plain sequence.
// WHICH source rows a band can read is not guessed: the set-up kernel reports, per cell row, an interval that
// contains the source row of every pixel of every cell in it (anchor row -+ the bound of the float32
// estimate's magnitude, apap_kernels.hip fast_record), and the host takes the union over the band's cell
// rows.  Meshes the set-up has no such interval for (irregular edges, cells wider than 254 pixels, a
// perspective denominator that changes sign inside a cell) wait for the whole image: the order of the
// transfers changes, never the bytes of the canvas.
namespace {

// (the overlapped path has three streams of its own and keeps its own error returns and its own drain, DrainStreams)
#define APAP_HIP_TRY(call)                                                              \
    do {                                                                                \
        const hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess) return apap::fail(APAP_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

struct PinGuard {       // hipHostRegister for the duration of a call
    void *p = nullptr;
    bool pin(const void *ptr, size_t bytes, unsigned flags = hipHostRegisterDefault) {
        // memory the caller already page-locked (hipHostMalloc, torch's pin_memory, its own hipHostRegister): nothing to do,
        // nothing to undo
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, ptr) == hipSuccess && at.type == hipMemoryTypeHost) {
            hipPointerAttribute_t last;
            if (hipPointerGetAttributes(&last, (const char *)ptr + bytes - 1) == hipSuccess && last.type == hipMemoryTypeHost) return true;
        }
        (void)hipGetLastError();
        if (hipHostRegister(const_cast<void *>(ptr), bytes, flags) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        p = const_cast<void *>(ptr);
        return true;
    }
    ~PinGuard() {
        if (p) (void)hipHostUnregister(p);
    }
};

int pipe_prepare(apap_ctx *pool, int dev, size_t n_events, size_t pinned_bytes) {
    if (pool->pipe_dev != dev) {     // streams and events belong to a device
        for (void *e : pool->events) (void)hipEventDestroy((hipEvent_t)e);
        pool->events.clear();
        for (void *&st : pool->streams) {
            if (st) (void)hipStreamDestroy((hipStream_t)st);
            st = nullptr;
        }
        pool->pipe_dev = dev;
    }
    for (void *&st : pool->streams)
        if (!st) {
            hipStream_t h;
            APAP_HIP_TRY(hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
            st = h;
        }
    while (pool->events.size() < n_events) {
        hipEvent_t e;
        APAP_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        pool->events.push_back(e);
    }
    if (pool->pinned_cap < pinned_bytes) {
        if (pool->pinned) (void)hipHostFree(pool->pinned);
        pool->pinned = nullptr;
        pool->pinned_cap = 0;
        APAP_HIP_TRY(hipHostMalloc(&pool->pinned, pinned_bytes, hipHostMallocDefault));
        pool->pinned_cap = pinned_bytes;
    }
    return APAP_OK;
}

struct DrainStreams {    // whatever way the function is left, nothing of it is still running
    apap_ctx *pool;
    ~DrainStreams() {
        for (void *st : pool->streams)
            if (st) (void)hipStreamSynchronize((hipStream_t)st);
    }
};

// rows of `total` in `parts` near-equal pieces: piece i = [cut(i), cut(i + 1))
inline int cut(int total, int parts, int i) { return (int)((long long)total * i / parts); }

// Returns APAP_OK and sets *done = true when the call was served here; *done = false (and APAP_OK) when the
// caller should take the plain sequential path (pinning refused, a mesh without the fast tables).
int warp_overlapped(apap_ctx *ctx, apap_ctx *pool, int dev, const uint8_t *img, int img_h, int img_w, const uint8_t *center,
                    int center_h, int center_w, const float *Hfwd, int mesh_rows, int mesh_cols, const double *mesh_w,
                    int n_w, const double *mesh_h, int n_h, int final_w, int final_h, int off_x, int off_y, uint8_t *out,
                    float *Hinv_out, const char *who, bool *done) {
    *done = false;
    const size_t img_bytes = (size_t)img_h * img_w * 3, out_bytes = (size_t)final_w * final_h * 3;
    const size_t cbytes = center ? (size_t)center_h * center_w * 3 : 0;
    if (img_bytes + out_bytes < (8u << 20)) return APAP_OK;      // small pairs: one copy each way is as good
    const int cells = mesh_rows * mesh_cols;
    // (chunks x bands x order were swept in round 4 - profiles/r04_pcie_duplex.txt: a plateau at 0.89-0.93 ms for 4-8 chunks and 4-8
    // bands; grid upload + set-up before the image chunks is worse whenever the inverses come back)
    const int chunks = (int)std::min<size_t>(16, std::max<size_t>(2, img_bytes / (3u << 20)));
    const int bands = (int)std::min<size_t>(16, std::max<size_t>(2, out_bytes / (3u << 20)));
    const size_t range_ints = (size_t)mesh_rows * 2 + 2;
    int rc = pipe_prepare(pool, dev, (size_t)2 * chunks + 2 * bands + 4, range_ints * sizeof(int) + 64);
    if (rc) return rc;
    // Only the three big buffers are pinned, and only when no two of them share a page.  History: with the grid and its
    // inverse pinned as well (numpy's `H.copy()` followed by `np.empty_like(H)`: back to back) one run of round 3 ended in a
    // GPU fault "write access to a read-only page", attributed then to the two registrations sharing a page.  Round 4's
    // stand-alone reproducer of exactly that layout (profiles/r04_hostreg_pages.txt, the program at git tag r05-hooks: both ranges
    // registered, DMA in both directions and at once, a kernel reading one and writing the other through the device
    // pointers, either unregistration order) runs clean on this stack: the shared page was NOT the cause, which stays
    // unknown (no log of the fault survived).  The rule is kept because it costs nothing: pinning 1.4 MB buys nothing (the
    // grid, its inverse and the edges travel as pageable copies on the kernel stream while the image chunks are already going
    // up), and page-disjoint registrations are the case every test exercises (tests/test_gpu_parity.py:
    // test_overlapped_host_warp_on_buffers_that_share_pages runs both layouts).
    auto pages_overlap = [](const void *a, size_t na, const void *b, size_t nb) {
        const uintptr_t pa0 = (uintptr_t)a >> 12, pa1 = ((uintptr_t)a + na - 1) >> 12;
        const uintptr_t pb0 = (uintptr_t)b >> 12, pb1 = ((uintptr_t)b + nb - 1) >> 12;
        return pa0 <= pb1 && pb0 <= pa1;
    };
    if (pages_overlap(img, img_bytes, out, out_bytes) ||
        (center && (pages_overlap(center, cbytes, out, out_bytes) || pages_overlap(center, cbytes, img, img_bytes))))
        return APAP_OK;
    PinGuard pin_img, pin_out, pin_center;
    if (!pin_img.pin(img, img_bytes) || !pin_out.pin(out, out_bytes) || (center && !pin_center.pin(center, cbytes))) return APAP_OK;

    const size_t work_bytes = apap_warp_workspace_bytes(mesh_rows, mesh_cols, final_w, final_h);
    void *d_H, *d_mw, *d_mh, *d_work, *d_status, *d_hinv = nullptr, *d_img, *d_out, *d_center = nullptr;
    if ((rc = slot_get(pool, S_H, (size_t)cells * 9 * sizeof(float), dev, &d_H))) return rc;
    if ((rc = slot_get(pool, S_MESHW, (size_t)n_w * sizeof(double), dev, &d_mw))) return rc;
    if ((rc = slot_get(pool, S_MESHH, (size_t)n_h * sizeof(double), dev, &d_mh))) return rc;
    if ((rc = slot_get(pool, S_WORK, work_bytes, dev, &d_work))) return rc;
    if ((rc = slot_get(pool, S_STATUS, sizeof(int), dev, &d_status))) return rc;
    if (Hinv_out && (rc = slot_get(pool, S_HINV, (size_t)cells * 9 * sizeof(float), dev, &d_hinv))) return rc;
    if ((rc = slot_get(pool, S_IMG, img_bytes, dev, &d_img))) return rc;
    if ((rc = slot_get(pool, S_OUT, out_bytes, dev, &d_out))) return rc;
    if (center && (rc = slot_get(pool, S_AUX, cbytes, dev, &d_center))) return rc;

    hipStream_t s_up = (hipStream_t)pool->streams[0], s_k = (hipStream_t)pool->streams[1], s_dn = (hipStream_t)pool->streams[2];
    hipEvent_t *ev = reinterpret_cast<hipEvent_t *>(pool->events.data());
    hipEvent_t *e_img = ev, *e_cen = ev + chunks, *e_band = ev + 2 * chunks, e_setup = ev[2 * chunks + bands];
    int *h_rng = (int *)pool->pinned;
    int status = 0;
    const DrainStreams drain{pool};     // declared after everything the streams read or write

    // upload stream: source rows (and the centre image's) in chunks, an event after each
    auto enqueue_uploads = [&]() -> int {
        for (int c = 0; c < chunks; ++c) {
            const size_t a = (size_t)cut(img_h, chunks, c) * img_w * 3, b = (size_t)cut(img_h, chunks, c + 1) * img_w * 3;
            if (b > a) APAP_HIP_TRY(hipMemcpyAsync((char *)d_img + a, img + a, b - a, hipMemcpyHostToDevice, s_up));
            APAP_HIP_TRY(hipEventRecord(e_img[c], s_up));
            if (center) {
                const size_t ca = (size_t)cut(center_h, chunks, c) * center_w * 3, cb = (size_t)cut(center_h, chunks, c + 1) * center_w * 3;
                if (cb > ca) APAP_HIP_TRY(hipMemcpyAsync((char *)d_center + ca, center + ca, cb - ca, hipMemcpyHostToDevice, s_up));
                APAP_HIP_TRY(hipEventRecord(e_cen[c], s_up));
            }
        }
        return APAP_OK;
    };
    if ((rc = enqueue_uploads())) return rc;

    // kernels stream: grid and edges up, set-up kernel, its source-row intervals back
    int *d_src_rows = nullptr;
    APAP_HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(int), s_k));
    APAP_HIP_TRY(hipMemcpyAsync(d_H, Hfwd, (size_t)cells * 9 * sizeof(float), hipMemcpyHostToDevice, s_k));
    APAP_HIP_TRY(hipMemcpyAsync(d_mw, mesh_w, (size_t)n_w * sizeof(double), hipMemcpyHostToDevice, s_k));
    APAP_HIP_TRY(hipMemcpyAsync(d_mh, mesh_h, (size_t)n_h * sizeof(double), hipMemcpyHostToDevice, s_k));
    {
        // where the intervals will live (the same layout the set-up uses); lower bounds start high, upper bounds low
        int *probe = nullptr;
        rc = apap::warp_phase(ctx, (const uint8_t *)d_img, img_h, img_w, (const uint8_t *)d_center, center_h, center_w,
                              (const float *)d_H, mesh_rows, mesh_cols, (const double *)d_mw, n_w, (const double *)d_mh, n_h,
                              final_w, final_h, off_x, off_y, (uint8_t *)d_out, (float *)d_hinv, d_work, work_bytes,
                              (int *)d_status, s_k, 0, 0, 0, &probe);
        if (rc) return rc;
        if (!probe) return APAP_OK;     // a mesh the fast tables do not cover: sequential path
        // one interleaved fill: even words (lower bounds) 0x7f7f7f7f, odd words (upper bounds) 0x80808080
        std::vector<int> init(range_ints);
        for (int r = 0; r < mesh_rows; ++r) {
            init[2 * r] = 0x7f7f7f7f;
            init[2 * r + 1] = (int)0x80808080u;
        }
        init[2 * mesh_rows] = init[2 * mesh_rows + 1] = 0;
        memcpy(h_rng, init.data(), range_ints * sizeof(int));
        // (h_rng is reused for the read-back below: the same stream, so the device has read it by then)
        APAP_HIP_TRY(hipMemcpyAsync(probe, h_rng, range_ints * sizeof(int), hipMemcpyHostToDevice, s_k));
    }
    rc = apap::warp_phase(ctx, (const uint8_t *)d_img, img_h, img_w, (const uint8_t *)d_center, center_h, center_w,
                          (const float *)d_H, mesh_rows, mesh_cols, (const double *)d_mw, n_w, (const double *)d_mh, n_h, final_w,
                          final_h, off_x, off_y, (uint8_t *)d_out, (float *)d_hinv, d_work, work_bytes, (int *)d_status, s_k, 0, 0,
                          apap::kWarpSetup, &d_src_rows);
    if (rc) return rc;
    APAP_HIP_TRY(hipMemcpyAsync(h_rng, d_src_rows, range_ints * sizeof(int), hipMemcpyDeviceToHost, s_k));
    APAP_HIP_TRY(hipEventRecord(e_setup, s_k));
    if (Hinv_out)
        APAP_HIP_TRY(hipMemcpyAsync(Hinv_out, d_hinv, (size_t)cells * 9 * sizeof(float), hipMemcpyDeviceToHost, s_k));

    // the intervals: which chunk must have landed before band b may run
    APAP_HIP_TRY(hipEventSynchronize(e_setup));
    // (the host's cell_row_of below is a binary search: valid on increasing edges only; the device's running-maximum table also
    // serves merely swapped edges, whose pixels all sit in ordinary cells and do not set the flag bit)
    const bool irregular = (h_rng[2 * mesh_rows] & 1) != 0 || !std::is_sorted(mesh_h, mesh_h + n_h);
    auto cell_row_of = [&](int y) {     // "first k with y < mesh_h[k]" - 1 on increasing edges
        const int k = (int)(std::upper_bound(mesh_h, mesh_h + n_h, (double)y) - mesh_h) - 1;
        return std::min(std::max(k, 0), mesh_rows - 1);
    };
    auto chunk_of_row = [&](int total, int row) {      // the chunk that holds `row`
        int c = (int)(((long long)row + 1) * chunks / std::max(total, 1));
        c = std::min(std::max(c, 0), chunks - 1);
        while (c > 0 && cut(total, chunks, c) > row) --c;
        while (c + 1 < chunks && cut(total, chunks, c + 1) <= row) ++c;
        return c;
    };
    for (int b = 0; b < bands; ++b) {
        const int y0 = cut(final_h, bands, b), y1 = cut(final_h, bands, b + 1);
        if (y1 <= y0) {
            APAP_HIP_TRY(hipEventRecord(e_band[b], s_k));
            continue;
        }
        int need = chunks - 1;      // without intervals: the whole image
        if (!irregular) {
            long long hi = -1;
            for (int r = cell_row_of(y0); r <= cell_row_of(y1 - 1); ++r) hi = std::max<long long>(hi, h_rng[2 * r + 1]);
            hi = std::min<long long>(hi + 1, img_h - 1);      // + 1: the gather's dword may reach into the next row
            need = hi < 0 ? 0 : chunk_of_row(img_h, (int)hi);
        }
        APAP_HIP_TRY(hipStreamWaitEvent(s_k, e_img[need], 0));
        if (center) {
            const int c_hi = std::min(std::max(y1 - 1 - off_y, 0), center_h - 1);
            APAP_HIP_TRY(hipStreamWaitEvent(s_k, e_cen[chunk_of_row(center_h, c_hi)], 0));
        }
        uint8_t *d_band = (uint8_t *)d_out + (size_t)y0 * final_w * 3;
        rc = apap::warp_phase(ctx, (const uint8_t *)d_img, img_h, img_w, (const uint8_t *)d_center, center_h, center_w,
                              (const float *)d_H, mesh_rows, mesh_cols, (const double *)d_mw, n_w, (const double *)d_mh, n_h,
                              final_w, final_h, off_x, off_y, d_band, nullptr, d_work, work_bytes, (int *)d_status, s_k, y0,
                              y1 - y0, apap::kWarpRows, nullptr);
        if (rc) return rc;
        APAP_HIP_TRY(hipEventRecord(e_band[b], s_k));
        APAP_HIP_TRY(hipStreamWaitEvent(s_dn, e_band[b], 0));
        APAP_HIP_TRY(hipMemcpyAsync(out + (size_t)y0 * final_w * 3, d_band, (size_t)(y1 - y0) * final_w * 3, hipMemcpyDeviceToHost, s_dn));
    }
    APAP_HIP_TRY(hipMemcpyAsync(h_rng, d_status, sizeof(int), hipMemcpyDeviceToHost, s_k));
    APAP_HIP_TRY(hipStreamSynchronize(s_k));
    status = h_rng[0];
    APAP_HIP_TRY(hipStreamSynchronize(s_dn));
    APAP_HIP_TRY(hipStreamSynchronize(s_up));
    *done = true;
    return status_to_code(status, who);
}

}  // namespace

// `h_bytes` = 4: the grid (and Hinv_out) is float32; 8: float64 (apap_local_warp_f64 only).
static int warp_common(apap_ctx *ctx, const uint8_t *img, int img_h, int img_w, const uint8_t *center, int center_h,
                       int center_w, const void *Hfwd, size_t h_bytes, int mesh_rows,
                       int mesh_cols, const double *mesh_w, int n_w, const double *mesh_h, int n_h,
                       int final_w, int final_h, int off_x, int off_y, uint8_t *out, void *Hinv_out,
                       double *coords, int device, const char *who) {
    if (!Hfwd || !mesh_w || !mesh_h) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    if (mesh_rows < 1 || mesh_cols < 1 || n_w < 1 || n_h < 1 || final_w < 1 || final_h < 1)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: bad size", who);
    int status = 0;   // the last download writes it
    HostCall call(ctx);
    int rc = call.select(device);
    if (rc) return rc;
    // (the overlapped path schedules its upload bands from src_rows, which bounds the TRUNCATED source row only: under bilinear
    // sampling the plain path)
    if (!coords && h_bytes == sizeof(float) && apap::opt(ctx, APAP_OPT_OVERLAP_PCIE) &&
        apap::opt(ctx, APAP_OPT_WARP_SAMPLING) == APAP_SAMPLING_NEAREST) {
        bool done = false;
        rc = warp_overlapped(ctx, call.pool(), call.dev(), img, img_h, img_w, center, center_h, center_w, (const float *)Hfwd,
                             mesh_rows, mesh_cols, mesh_w, n_w, mesh_h, n_h, final_w, final_h, off_x, off_y, out, (float *)Hinv_out,
                             who, &done);
        if (rc || done) return rc;
    }
    const int cells = mesh_rows * mesh_cols;
    const size_t pixels = (size_t)final_w * final_h;
    const Part H = call.slot(S_H, (size_t)cells * 9 * h_bytes);
    const Part mw = call.slot(S_MESHW, (size_t)n_w * sizeof(double));
    const Part mh = call.slot(S_MESHH, (size_t)n_h * sizeof(double));
    const Part work = call.slot(S_WORK, apap_warp_workspace_bytes(mesh_rows, mesh_cols, final_w, final_h));
    const Part d_status = call.slot(S_STATUS, sizeof(int));
    const Part hinv = Hinv_out ? call.slot(S_HINV, H.bytes) : Part{};
    void *d_hinv = Hinv_out ? hinv.as<void>() : nullptr;
    call.zero(d_status);
    call.up(H, Hfwd);
    call.up(mw, mesh_w);
    call.up(mh, mesh_h);
    if (coords) {
        const Part xy = call.slot(S_OUT, pixels * 2 * sizeof(double));
        if ((rc = call.rc())) return rc;
        rc = apap_warp_coords_device(ctx, H.as<const float>(), mesh_rows, mesh_cols, mw.as<const double>(), n_w,
                                     mh.as<const double>(), n_h, final_w, final_h, off_x, off_y, xy.as<double>(), work.as<void>(),
                                     work.bytes, d_status.as<int>(), call.stream());
        if (rc) return rc;
        call.down(coords, xy);
    } else {
        const Part d_img = call.slot(S_IMG, (size_t)img_h * img_w * 3);
        const Part d_out = call.slot(S_OUT, pixels * 3);
        call.up(d_img, img);
        Part d_center{};
        if (center) {
            d_center = call.slot(S_AUX, (size_t)center_h * center_w * 3);
            call.up(d_center, center);
        }
        if ((rc = call.rc())) return rc;
        if (center) {
            rc = apap_stitch_device(ctx, d_img.as<const uint8_t>(), img_h, img_w, d_center.as<const uint8_t>(), center_h, center_w,
                                    H.as<const float>(), mesh_rows, mesh_cols, mw.as<const double>(), n_w, mh.as<const double>(),
                                    n_h, final_w, final_h, off_x, off_y, d_out.as<uint8_t>(), (float *)d_hinv, work.as<void>(),
                                    work.bytes, d_status.as<int>(), call.stream());
        } else if (h_bytes == sizeof(double)) {
            rc = apap_warp_f64_device(ctx, d_img.as<const uint8_t>(), img_h, img_w, H.as<const double>(), mesh_rows, mesh_cols,
                                      mw.as<const double>(), n_w, mh.as<const double>(), n_h, final_w, final_h, off_x, off_y,
                                      d_out.as<uint8_t>(), (double *)d_hinv, work.as<void>(), work.bytes, d_status.as<int>(),
                                      call.stream());
        } else {
            rc = apap_warp_device(ctx, d_img.as<const uint8_t>(), img_h, img_w, H.as<const float>(), mesh_rows, mesh_cols,
                                  mw.as<const double>(), n_w, mh.as<const double>(), n_h, final_w, final_h, off_x, off_y,
                                  d_out.as<uint8_t>(), (float *)d_hinv, work.as<void>(), work.bytes, d_status.as<int>(),
                                  call.stream());
        }
        if (rc) return rc;
        call.down(out, d_out);
        if (Hinv_out) call.down(Hinv_out, hinv);
    }
    call.down(&status, d_status);
    if ((rc = call.wait())) return rc;
    return status_to_code(status, who);
}

int apap_local_warp(apap_ctx *ctx, const uint8_t *img, int img_h, int img_w, const float *Hfwd, int mesh_rows,
                    int mesh_cols, const double *mesh_w, int n_w, const double *mesh_h, int n_h,
                    int final_w, int final_h, int off_x, int off_y, uint8_t *out, float *Hinv_out,
                    int device) {
    if (!img || !out) return apap::fail(APAP_ERR_INVALID_ARG, "apap_local_warp: null image");
    if (img_h < 1 || img_w < 1) return apap::fail(APAP_ERR_INVALID_ARG, "apap_local_warp: bad image size");
    return warp_common(ctx, img, img_h, img_w, nullptr, 0, 0, Hfwd, sizeof(float), mesh_rows, mesh_cols, mesh_w, n_w, mesh_h, n_h,
                       final_w, final_h, off_x, off_y, out, Hinv_out, nullptr, device, "apap_local_warp");
}

int apap_local_warp_f64(apap_ctx *ctx, const uint8_t *img, int img_h, int img_w, const double *Hfwd, int mesh_rows,
                        int mesh_cols, const double *mesh_w, int n_w, const double *mesh_h, int n_h,
                        int final_w, int final_h, int off_x, int off_y, uint8_t *out, double *Hinv_out,
                        int device) {
    if (!img || !out) return apap::fail(APAP_ERR_INVALID_ARG, "apap_local_warp_f64: null image");
    if (img_h < 1 || img_w < 1) return apap::fail(APAP_ERR_INVALID_ARG, "apap_local_warp_f64: bad image size");
    return warp_common(ctx, img, img_h, img_w, nullptr, 0, 0, Hfwd, sizeof(double), mesh_rows, mesh_cols, mesh_w, n_w, mesh_h,
                       n_h, final_w, final_h, off_x, off_y, out, Hinv_out, nullptr, device, "apap_local_warp_f64");
}

int apap_local_stitch(apap_ctx *ctx, const uint8_t *img, int img_h, int img_w, const uint8_t *center, int center_h,
                      int center_w, const float *Hfwd, int mesh_rows, int mesh_cols,
                      const double *mesh_w, int n_w, const double *mesh_h, int n_h, int final_w,
                      int final_h, int off_x, int off_y, uint8_t *out, float *Hinv_out, int device) {
    if (!img || !out || !center) return apap::fail(APAP_ERR_INVALID_ARG, "apap_local_stitch: null image");
    if (img_h < 1 || img_w < 1 || center_h < 1 || center_w < 1)
        return apap::fail(APAP_ERR_INVALID_ARG, "apap_local_stitch: bad image size");
    return warp_common(ctx, img, img_h, img_w, center, center_h, center_w, Hfwd, sizeof(float), mesh_rows, mesh_cols, mesh_w, n_w,
                       mesh_h, n_h, final_w, final_h, off_x, off_y, out, Hinv_out, nullptr, device, "apap_local_stitch");
}

int apap_warp_coords(apap_ctx *ctx, const float *Hfwd, int mesh_rows, int mesh_cols, const double *mesh_w, int n_w,
                     const double *mesh_h, int n_h, int final_w, int final_h, int off_x, int off_y,
                     double *coords, int device) {
    if (!coords) return apap::fail(APAP_ERR_INVALID_ARG, "apap_warp_coords: null output");
    return warp_common(ctx, nullptr, 0, 0, nullptr, 0, 0, Hfwd, sizeof(float), mesh_rows, mesh_cols, mesh_w, n_w, mesh_h, n_h,
                       final_w, final_h, off_x, off_y, nullptr, nullptr, coords, device, "apap_warp_coords");
}

int apap_invert_normalize_flatten(apap_ctx *ctx, const float *H, int cells, double *out, int device) {
    if (!H || !out || cells < 1) return apap::fail(APAP_ERR_INVALID_ARG, "apap_invert_normalize_flatten: bad argument");
    int status = 0;   // the last download writes it
    HostCall call(ctx);
    int rc = call.select(device);
    if (rc) return rc;
    const Part d_H = call.slot(S_H, (size_t)cells * 9 * sizeof(float));
    const Part d_out = call.slot(S_AUX, (size_t)cells * 9 * sizeof(double));
    const Part d_status = call.slot(S_STATUS, sizeof(int));
    call.zero(d_status);
    call.up(d_H, H);
    if ((rc = call.rc())) return rc;
    rc = apap_flatten_device(ctx, d_H.as<const float>(), cells, d_out.as<double>(), d_status.as<int>(), call.stream());
    if (rc) return rc;
    call.down(out, d_out);
    call.down(&status, d_status);
    if ((rc = call.wait())) return rc;
    return status_to_code(status, "apap_invert_normalize_flatten");
}

int apap_uniform_blend(apap_ctx *ctx, const uint8_t *img1, const uint8_t *img2, int h, int w, uint8_t *out,
                       int device) {
    if (!img1 || !img2 || !out || h < 1 || w < 1) return apap::fail(APAP_ERR_INVALID_ARG, "apap_uniform_blend: bad argument");
    HostCall call(ctx);
    int rc = call.select(device);
    if (rc) return rc;
    const size_t bytes = (size_t)h * w * 3;
    const Part a = call.slot(S_IMG, bytes), b = call.slot(S_AUX, bytes), o = call.slot(S_OUT, bytes);
    call.up(a, img1);
    call.up(b, img2);
    if ((rc = call.rc())) return rc;
    rc = apap_blend_device(ctx, a.as<const uint8_t>(), b.as<const uint8_t>(), h, w, o.as<uint8_t>(), call.stream());
    if (rc) return rc;
    call.down(out, o);
    return call.wait();
}

int apap_equalize_hist(apap_ctx *ctx, const uint8_t *img, int h, int w, int channels, uint8_t *out, int device) {
    if (!img || !out || h < 1 || w < 1 || channels < 1 || channels > 4)
        return apap::fail(APAP_ERR_INVALID_ARG, "apap_equalize_hist: bad argument");
    HostCall call(ctx);
    int rc = call.select(device);
    if (rc) return rc;
    const size_t bytes = (size_t)h * w * channels;
    const Part a = call.slot(S_IMG, bytes), o = call.slot(S_OUT, bytes);
    const Part work = call.slot(S_WORK, apap_equalize_workspace_bytes(channels));
    call.up(a, img);
    call.zero(work);   // the device form wants it zero on entry, and the pool's S_WORK holds what any other call left: per call
    if ((rc = call.rc())) return rc;
    rc = apap_equalize_hist_device(ctx, a.as<const uint8_t>(), h, w, channels, o.as<uint8_t>(), work.as<void>(), work.bytes,
                                   call.stream());
    if (rc) return rc;
    call.down(out, o);
    return call.wait();
}

int apap_find_homography_ransac(apap_ctx *ctx, const float *src, const float *dst, int n, double thresh, int iterations,
                                unsigned long long seed, double *H_out, uint8_t *mask_out, int *inliers_out,
                                int device) {
    if (!src || !dst || !H_out || !mask_out || !inliers_out)
        return apap::fail(APAP_ERR_INVALID_ARG, "apap_find_homography_ransac: null argument");
    if (n < 4) return apap::fail(APAP_ERR_INVALID_ARG, "apap_find_homography_ransac: n=%d, a homography needs 4 points", n);
    int result[2] = {0, 0};
    {
        // This scope ends the call, and so releases the pool, before the re-fit below: apap_local_homography takes the
        // same pool's mutex, which is not recursive.
        HostCall call(ctx);
        int rc = call.select(device);
        if (rc) return rc;
        const size_t pt_bytes = (size_t)n * 2 * sizeof(float);
        const Part d_src = call.slot(S_IMG, pt_bytes), d_dst = call.slot(S_AUX, pt_bytes);
        const Part work = call.slot(S_WORK, apap_ransac_workspace_bytes(n, iterations));
        const Part d_H = call.slot(S_DENORM, 9 * sizeof(double));
        const Part d_mask = call.slot(S_OUT, (size_t)n);
        const Part d_result = call.slot(S_STATUS, sizeof(result));
        call.up(d_src, src);
        call.up(d_dst, dst);
        if ((rc = call.rc())) return rc;
        rc = apap_ransac_device(ctx, d_src.as<const float>(), d_dst.as<const float>(), n, thresh, iterations, seed, d_H.as<double>(),
                                d_mask.as<uint8_t>(), d_result.as<int>(), work.as<void>(), work.bytes, call.stream());
        if (rc) return rc;
        call.down(mask_out, d_mask);
        call.down(result, d_result);
        if ((rc = call.wait())) return rc;
    }
    *inliers_out = result[1];
    if (result[1] < 4) {  // cv.findHomography returns no model
        memset(mask_out, 0, (size_t)n);
        return APAP_OK;
    }
    // re-fit to the inliers with the hot path's own normalised DLT: one cell, every weight 1
    std::vector<float> s_in, d_in;
    s_in.reserve((size_t)2 * result[1]);
    d_in.reserve((size_t)2 * result[1]);
    for (int k = 0; k < n; ++k) {
        if (!mask_out[k]) continue;
        s_in.push_back(src[2 * k]); s_in.push_back(src[2 * k + 1]);
        d_in.push_back(dst[2 * k]); d_in.push_back(dst[2 * k + 1]);
    }
    const double vertex[2] = {0.0, 0.0};
    float H32[9];
    const int rc = apap_local_homography(ctx, s_in.data(), d_in.data(), (int)(s_in.size() / 2), vertex, 1, 1, 1.0, 1.0, H32,
                                         nullptr, device);
    if (rc) return rc;
    for (int i = 0; i < 9; ++i) H_out[i] = (double)H32[i];
    return APAP_OK;
}

int apap_find_fundamental_ransac_batch(apap_ctx *ctx, const float *src, const float *dst, const int *pair_offset, int n_pairs,
                                       double thresh, int iterations, unsigned long long seed, double *F_out, uint8_t *mask_out,
                                       int *inliers_out, int device) {
    const char *who = "apap_find_fundamental_ransac_batch";
    if (!src || !dst || !F_out || !mask_out || !inliers_out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    int rc = apap::fundamental_check(pair_offset, n_pairs, thresh, iterations, who);
    if (rc) return rc;
    std::vector<int> result((size_t)n_pairs * 2, 0);   // before the HostCall: a download writes it
    const size_t first = (size_t)pair_offset[0], N = (size_t)pair_offset[n_pairs] - first;   // the device arrays start at the first pair
    const std::vector<int> rel = relative_offsets(pair_offset, n_pairs);
    {
        HostCall call(ctx);
        if ((rc = call.select(device))) return rc;
        Layout io = call.layout(S_AUX);
        const Part d_src = io.take(N * 2 * sizeof(float)), d_dst = io.take(N * 2 * sizeof(float));
        const Part d_F = io.take((size_t)n_pairs * 9 * sizeof(double)), d_mask = io.take(N);
        const Part d_result = io.take(result.size() * sizeof(int));
        call.alloc(io);
        const Part work = call.slot(S_WORK, apap_fundamental_workspace_bytes((int)N, n_pairs, iterations));
        call.up(d_src, src + first * 2);
        call.up(d_dst, dst + first * 2);
        if ((rc = call.rc())) return rc;
        rc = apap_fundamental_batch_device(ctx, d_src.as<const float>(), d_dst.as<const float>(), rel.data(), n_pairs, thresh, iterations,
                                           seed, d_F.as<double>(), d_mask.as<uint8_t>(), d_result.as<int>(), work.as<void>(), work.bytes,
                                           call.stream());
        if (rc) return rc;
        call.down(F_out, d_F);
        call.down(mask_out + first, d_mask);
        call.down(result.data(), d_result);
        if ((rc = call.wait())) return rc;
    }
    for (int p = 0; p < n_pairs; ++p) {
        inliers_out[p] = result[2 * (size_t)p + 1];
        if (std::isnan(F_out[9 * (size_t)p]))   // no model: cv.findFundamentalMat returns None
            memset(mask_out + pair_offset[p], 0, (size_t)(pair_offset[p + 1] - pair_offset[p]));
    }
    return APAP_OK;
}

int apap_find_fundamental_ransac(apap_ctx *ctx, const float *src, const float *dst, int n, double thresh, int iterations,
                                 unsigned long long seed, double *F_out, uint8_t *mask_out, int *inliers_out, int device) {
    const int off[2] = {0, n};
    return apap_find_fundamental_ransac_batch(ctx, src, dst, off, 1, thresh, iterations, seed, F_out, mask_out, inliers_out, device);
}

// ---- notch denoising (apap_denoise.hip): every argument is checked before a device is looked for
int apap_fft2(apap_ctx *ctx, const double *in, double *out, int planes, int h, int w, int inverse, int device) {
    const char *who = "apap_fft2";
    int rc = apap::fft_check(planes, h, w, who);
    if (rc) return rc;
    if (!in || !out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    const Part d_f = call.slot(S_OUT, (size_t)planes * h * w * 16), work = call.slot(S_WORK, apap_fft2_workspace_bytes(planes, h, w));
    call.up(d_f, in);
    if ((rc = call.rc())) return rc;
    rc = apap_fft2_device(ctx, d_f.as<const double>(), d_f.as<double>(), planes, h, w, inverse, work.as<void>(), work.bytes, call.stream());
    if (rc) return rc;
    call.down(out, d_f);
    return call.wait();
}

int apap_notch_spectrum(apap_ctx *ctx, double *f, int planes, int h, int w, int spacing, int r, int sn, int device) {
    const char *who = "apap_notch_spectrum";
    if (planes < 1 || planes > apap::kDenoiseMaxPlanes || h < 1 || w < 1 || h > APAP_FFT_MAX_LENGTH || w > APAP_FFT_MAX_LENGTH)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: %d planes of %d x %d (1 .. %d planes, sides 1 .. %d)", who, planes, h, w,
                          apap::kDenoiseMaxPlanes, APAP_FFT_MAX_LENGTH);
    int rc = apap::notch_check(spacing, r, sn, who);
    if (rc) return rc;
    if (!f) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    const Part d_f = call.slot(S_OUT, (size_t)planes * h * w * 16);
    call.up(d_f, f);
    if ((rc = call.rc())) return rc;
    if ((rc = apap_notch_spectrum_device(ctx, d_f.as<double>(), planes, h, w, spacing, r, sn, call.stream()))) return rc;
    call.down(f, d_f);
    return call.wait();
}

int apap_notch_denoise(apap_ctx *ctx, const uint8_t *imgs, int n_images, int h, int w, int channels, int equalize, int spacing,
                       int r, int sn, int out_type, void *out, int device) {
    const char *who = "apap_notch_denoise";
    int rc = apap::denoise_check(n_images, h, w, channels, spacing, r, sn, out_type, who);
    if (rc) return rc;
    if (!imgs || !out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    const size_t values = (size_t)n_images * h * w * channels;
    const Part d_img = call.slot(S_IMG, values), d_out = call.slot(S_OUT, values * (out_type == APAP_DENOISE_OUT_U8 ? 1 : 8));
    const Part work = call.slot(S_WORK, apap_notch_denoise_workspace_bytes(n_images, h, w, channels));
    call.up(d_img, imgs);
    if ((rc = call.rc())) return rc;
    rc = apap_notch_denoise_device(ctx, d_img.as<const uint8_t>(), n_images, h, w, channels, equalize, spacing, r, sn, out_type,
                                   d_out.as<void>(), work.as<void>(), work.bytes, call.stream());
    if (rc) return rc;
    call.down(out, d_out);
    return call.wait();
}

// ---- co-visibility tracks and triangulation (apap_sfm.hip): every argument is checked before a device is looked for
int apap_covis_tracks(apap_ctx *ctx, const float *pts, const int *idx, const int *view_offset, int n_views, float eps, int *table_out,
                      float *track_pts_out, int *point_track_out, int *n_tracks_out, int device) {
    const char *who = "apap_covis_tracks";
    int rc = apap::covis_check(view_offset, n_views, eps, who);
    if (rc) return rc;
    if (!pts || !idx || !table_out || !track_pts_out || !point_track_out || !n_tracks_out)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    int result[2] = {0, 0};   // tracks, status: downloads write it
    const size_t N = (size_t)view_offset[n_views];
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    Layout io = call.layout(S_AUX);
    const Part d_pts = io.take(N * 2 * sizeof(float)), d_idx = io.take(N * sizeof(int)), d_table = io.take(N * n_views * sizeof(int));
    const Part d_tpts = io.take(N * 2 * sizeof(float)), d_ptrack = io.take(N * sizeof(int)), d_result = io.take(sizeof(result));
    call.alloc(io);
    const Part work = call.slot(S_WORK, apap_covis_workspace_bytes((int)N, n_views));
    call.up(d_pts, pts);
    call.up(d_idx, idx);
    call.zero(d_result);
    if ((rc = call.rc())) return rc;
    rc = apap_covis_tracks_device(ctx, d_pts.as<const float>(), d_idx.as<const int>(), view_offset, n_views, eps, d_table.as<int>(),
                                  d_tpts.as<float>(), d_ptrack.as<int>(), d_result.as<int>(), d_result.as<int>() + 1, work.as<void>(),
                                  work.bytes, call.stream());
    if (rc) return rc;
    call.down(result, d_result);
    if ((rc = call.wait())) return rc;
    if (result[1] & APAP_STATUS_COVIS_BOUND) return apap::fail(APAP_ERR_HIP, "%s: the resolver reached its round bound", who);
    // only the rows that exist: what lies behind them in the caller's arrays stays
    const size_t T = (size_t)result[0];
    call.down(table_out, d_table.first(T * n_views * sizeof(int)));
    call.down(track_pts_out, d_tpts.first(T * 2 * sizeof(float)));
    call.down(point_track_out, d_ptrack);
    *n_tracks_out = result[0];
    return call.wait();
}

int apap_triangulate_rays(apap_ctx *ctx, const double *origins, const double *dirs, const int *ray_offset, int n_tracks, double *X_out,
                          double *lam_min_out, int *n_rays_out, int device) {
    const char *who = "apap_triangulate_rays";
    if (n_tracks < 0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: %d tracks (>= 0)", who, n_tracks);
    if (!origins || !dirs || !ray_offset || !X_out || !lam_min_out || !n_rays_out)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    if (ray_offset[0] != 0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: ray_offset[0] = %d (the rays start at 0)", who, ray_offset[0]);
    for (int k = 0; k < n_tracks; ++k)
        if (ray_offset[k + 1] < ray_offset[k]) return apap::fail(APAP_ERR_INVALID_ARG, "%s: ray_offset is not ascending at track %d", who, k);
    HostCall call(ctx);
    int rc = call.select(device);
    if (rc) return rc;
    const size_t R = (size_t)ray_offset[n_tracks], T = (size_t)n_tracks;
    Layout io = call.layout(S_AUX);
    const Part d_o = io.take(R * 3 * sizeof(double)), d_d = io.take(R * 3 * sizeof(double)), d_off = io.take((T + 1) * sizeof(int));
    const Part d_X = io.take(T * 3 * sizeof(double)), d_lam = io.take(T * sizeof(double)), d_n = io.take(T * sizeof(int));
    call.alloc(io);
    call.up(d_o, origins);
    call.up(d_d, dirs);
    call.up(d_off, ray_offset);
    if ((rc = call.rc())) return rc;
    rc = apap_triangulate_rays_device(ctx, d_o.as<const double>(), d_d.as<const double>(), d_off.as<const int>(), (int)R, n_tracks,
                                      d_X.as<double>(), d_lam.as<double>(), d_n.as<int>(), call.stream());
    if (rc) return rc;
    call.down(X_out, d_X);
    call.down(lam_min_out, d_lam);
    call.down(n_rays_out, d_n);
    return call.wait();
}

int apap_triangulate_tracks(apap_ctx *ctx, const int *table, const float *track_pts, int n_tracks, int n_views, const float *dst_pts,
                            const int *dst_offset, const double *Kinv, const double *R, const double *origins, int n_cams,
                            int center_cam, const int *view_cam, int min_views, double *X_out, double *lam_min_out, int *n_rays_out,
                            int device) {
    const char *who = "apap_triangulate_tracks";
    int rc = apap::triangulate_tracks_check(n_tracks, n_views, dst_offset, n_cams, center_cam, view_cam, min_views, who);
    if (rc) return rc;
    if (!table || !track_pts || !dst_pts || !Kinv || !R || !origins || !X_out || !lam_min_out || !n_rays_out)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    const size_t T = (size_t)n_tracks, D = (size_t)dst_offset[n_views];
    Layout io = call.layout(S_AUX);
    const Part d_table = io.take(T * n_views * sizeof(int)), d_tpts = io.take(T * 2 * sizeof(float)), d_dst = io.take(D * 2 * sizeof(float));
    const Part d_K = io.take(9 * sizeof(double)), d_R = io.take((size_t)n_cams * 9 * sizeof(double));
    const Part d_o = io.take((size_t)n_cams * 3 * sizeof(double));
    const Part d_X = io.take(T * 3 * sizeof(double)), d_lam = io.take(T * sizeof(double)), d_n = io.take(T * sizeof(int));
    call.alloc(io);
    call.up(d_table, table);
    call.up(d_tpts, track_pts);
    call.up(d_dst, dst_pts);
    call.up(d_K, Kinv);
    call.up(d_R, R);
    call.up(d_o, origins);
    if ((rc = call.rc())) return rc;
    rc = apap_triangulate_tracks_device(ctx, d_table.as<const int>(), d_tpts.as<const float>(), nullptr, n_tracks, n_views,
                                        d_dst.as<const float>(), dst_offset, d_K.as<const double>(), d_R.as<const double>(),
                                        d_o.as<const double>(), n_cams, center_cam, view_cam, min_views, d_X.as<double>(),
                                        d_lam.as<double>(), d_n.as<int>(), call.stream());
    if (rc) return rc;
    call.down(X_out, d_X);
    call.down(lam_min_out, d_lam);
    call.down(n_rays_out, d_n);
    return call.wait();
}

// ---- dehazing (apap_dehaze.hip): one host-buffer call for its four entry points; an output that is NULL is not computed
static int dehaze_host(apap_ctx *ctx, const uint8_t *imgs, int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q,
                       int refine, int eps, uint8_t *dark, uint8_t *A, uint16_t *t, uint8_t *J, int device, const char *who) {
    int rc = apap::dehaze_check(n_images, h, w, channels, radius, omega_q, t0_q, refine, eps, who);
    if (rc) return rc;
    if (!imgs || !(dark || A || t || J)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    const size_t N = (size_t)n_images * h * w;
    const Part d_img = call.slot(S_IMG, N * channels);
    Layout lay = call.layout(S_OUT);
    const Part d_dark = lay.take(dark ? N : 0), d_A = lay.take(A ? (size_t)n_images * channels : 0), d_t = lay.take(t ? N * 2 : 0),
               d_J = lay.take(J ? N * channels : 0);
    call.alloc(lay);
    const Part work = call.slot(S_WORK, apap_dehaze_workspace_bytes(n_images, h, w, channels, refine));
    call.up(d_img, imgs);
    if ((rc = call.rc())) return rc;
    rc = apap::dehaze_run(d_img.as<const uint8_t>(), n_images, h, w, channels, radius, omega_q, t0_q, refine, eps,
                          dark ? d_dark.as<uint8_t>() : nullptr, A ? d_A.as<uint8_t>() : nullptr, t ? d_t.as<uint16_t>() : nullptr,
                          J ? d_J.as<uint8_t>() : nullptr, work.as<void>(), work.bytes, call.stream(), who);
    if (rc) return rc;
    if (dark) call.down(dark, d_dark);
    if (A) call.down(A, d_A);
    if (t) call.down(t, d_t);
    if (J) call.down(J, d_J);
    return call.wait();
}

int apap_dark_channel(apap_ctx *ctx, const uint8_t *imgs, int n_images, int h, int w, int channels, int radius, uint8_t *dark, int device) {
    if (!dark) return apap::fail(APAP_ERR_INVALID_ARG, "apap_dark_channel: null argument");
    return dehaze_host(ctx, imgs, n_images, h, w, channels, radius, 0, 1, 0, 1, dark, nullptr, nullptr, nullptr, device, "apap_dark_channel");
}

int apap_atmospheric_light(apap_ctx *ctx, const uint8_t *imgs, int n_images, int h, int w, int channels, int radius, uint8_t *A, int device) {
    if (!A) return apap::fail(APAP_ERR_INVALID_ARG, "apap_atmospheric_light: null argument");
    return dehaze_host(ctx, imgs, n_images, h, w, channels, radius, 0, 1, 0, 1, nullptr, A, nullptr, nullptr, device, "apap_atmospheric_light");
}

int apap_transmission(apap_ctx *ctx, const uint8_t *imgs, int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q,
                      int refine, int eps, uint16_t *t, int device) {
    if (!t) return apap::fail(APAP_ERR_INVALID_ARG, "apap_transmission: null argument");
    return dehaze_host(ctx, imgs, n_images, h, w, channels, radius, omega_q, t0_q, refine, eps, nullptr, nullptr, t, nullptr, device,
                       "apap_transmission");
}

int apap_dehaze(apap_ctx *ctx, const uint8_t *imgs, int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q, int refine,
                int eps, uint8_t *out, uint16_t *t, uint8_t *A, int device) {
    if (!out) return apap::fail(APAP_ERR_INVALID_ARG, "apap_dehaze: null argument");
    return dehaze_host(ctx, imgs, n_images, h, w, channels, radius, omega_q, t0_q, refine, eps, nullptr, A, t, out, device, "apap_dehaze");
}

}  // extern "C"

// ------------------------------------------------------------------ spectral weights (spectral_method.py:66-133)
// The inputs and outputs of one call share one pooled device buffer (parts 256-byte aligned); the Lanczos workspace is a
// second one.
namespace {
struct SpecIo {
    Part src, dst, c, o, F, Hg, mask, seg, rm, om, info, M;
};
SpecIo spec_io(Layout &io, int n, bool dense) {
    const size_t pts = (size_t)n * 2 * sizeof(float), feats = (size_t)n * APAP_SPECTRAL_DIM * sizeof(float);
    SpecIo p;
    p.src = io.take(pts);
    p.dst = io.take(pts);
    p.c = io.take(feats);
    p.o = io.take(feats);
    p.F = io.take(9 * sizeof(double));
    p.Hg = io.take(9 * sizeof(float));
    p.mask = io.take((size_t)n * sizeof(float));
    p.seg = io.take((size_t)n * sizeof(double));
    p.rm = io.take((size_t)n * sizeof(float));
    p.om = io.take((size_t)n * sizeof(float));
    p.info = io.take(APAP_SPECTRAL_INFO * sizeof(double));
    p.M = io.take(dense ? (size_t)n * n * sizeof(double) : 0);
    return p;
}

void spec_upload(HostCall &call, const SpecIo &p, const float *src, const float *dst, const float *c_feats, const float *o_feats,
                 const double *F) {
    call.up(p.src, src);
    call.up(p.dst, dst);
    call.up(p.c, c_feats);
    call.up(p.o, o_feats);
    call.up(p.F, F);
}
}  // namespace

extern "C" {

int apap_spectral_weights(apap_ctx *ctx, const float *src, const float *dst, const float *c_feats, const float *o_feats, int n,
                          const double *F, const double *params, const float *Hg_or_null, const float *mask_in_or_null,
                          double *segment_out, float *ransac_mask_out, float *original_mask_out, double *info_out, int device) {
    if (!src || !dst || !c_feats || !o_feats || !F || !params || !segment_out || !ransac_mask_out || !original_mask_out || !info_out)
        return apap::fail(APAP_ERR_INVALID_ARG, "apap_spectral_weights: null argument");
    if (!Hg_or_null && !mask_in_or_null)
        return apap::fail(APAP_ERR_INVALID_ARG, "apap_spectral_weights: no initial mask (neither Hg nor a mask): the reference's "
                                                "init_ransac=False path fails on `None *= float` (spectral_method.py:131)");
    if (n < 1 || n > (1 << 26)) return apap::fail(APAP_ERR_INVALID_ARG, "apap_spectral_weights: n=%d (need 1 .. 2^26 matches)", n);
    HostCall call(ctx);
    int rc = call.select(device);
    if (rc) return rc;
    Layout io = call.layout(S_AUX);
    const SpecIo p = spec_io(io, n, false);
    call.alloc(io);
    const Part work = call.slot(S_WORK, apap_spectral_workspace_bytes(n));
    spec_upload(call, p, src, dst, c_feats, o_feats, F);
    if (Hg_or_null) call.up(p.Hg, Hg_or_null);
    else call.up(p.mask, mask_in_or_null);
    if ((rc = call.rc())) return rc;
    rc = apap::spectral_run(ctx, p.src.as<const float>(), p.dst.as<const float>(), p.c.as<const float>(), p.o.as<const float>(), n,
                            p.F.as<const double>(), params, Hg_or_null ? p.Hg.as<const float>() : nullptr,
                            Hg_or_null ? nullptr : p.mask.as<const float>(), p.seg.as<double>(), p.rm.as<float>(), p.om.as<float>(),
                            p.info.as<double>(), nullptr, work.as<void>(), work.bytes, call.stream(), 1);
    if (rc) return rc;
    call.down(segment_out, p.seg);
    call.down(ransac_mask_out, p.rm);
    call.down(original_mask_out, p.om);
    call.down(info_out, p.info);
    return call.wait();
}

int apap_spectral_affinity(apap_ctx *ctx, const float *src, const float *dst, const float *c_feats, const float *o_feats, int n,
                           const double *F, const double *params, double *M_out, int device) {
    if (!src || !dst || !c_feats || !o_feats || !F || !params || !M_out)
        return apap::fail(APAP_ERR_INVALID_ARG, "apap_spectral_affinity: null argument");
    if (n < 1 || n > 8192) return apap::fail(APAP_ERR_INVALID_ARG, "apap_spectral_affinity: n=%d (the dense M is for 1 .. 8192 matches)", n);
    HostCall call(ctx);
    int rc = call.select(device);
    if (rc) return rc;
    Layout io = call.layout(S_AUX);
    const SpecIo p = spec_io(io, n, true);
    call.alloc(io);
    const Part work = call.slot(S_WORK, apap_spectral_workspace_bytes(n));
    spec_upload(call, p, src, dst, c_feats, o_feats, F);
    if ((rc = call.rc())) return rc;
    rc = apap::spectral_affinity_run(p.src.as<const float>(), p.dst.as<const float>(), p.c.as<const float>(), p.o.as<const float>(), n,
                                     p.F.as<const double>(), params, p.M.as<double>(), work.as<void>(), work.bytes, call.stream());
    if (rc) return rc;
    call.down(M_out, p.M);
    return call.wait();
}

}  // extern "C"

// ------------------------------------------------------------------ M-step and EM loop (spectral_method.py:165-241)
// The M-step's own decoding of its status bits (status_to_code above keeps its three): a degenerate selection is
// APAP_ERR_INVALID_ARG, a zero pivot of the inverse APAP_ERR_SINGULAR (numpy: LinAlgError); the iteration cap is reported
// in the info block only.
namespace {
int model_status_code(int status, const char *who, int round) {
    if (status & APAP_STATUS_MODEL_DEGENERATE)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: round %d: fewer than 4 selected matches, or they do not determine a homography "
                                                "(rank-deficient system)", who, round);
    if (status & APAP_STATUS_SINGULAR) return apap::fail(APAP_ERR_SINGULAR, "%s: round %d: Singular matrix", who, round);
    return APAP_OK;
}

}  // namespace

extern "C" {

int apap_model_solve(apap_ctx *ctx, const float *pts_c, const float *pts_o, const float *weights, int n, const double *params,
                     float *H_out, double *info_out, int device) {
    const char *who = "apap_model_solve";
    // the info block is NaN until the kernels have written it: an early return leaves no stale count or status behind
    if (info_out) std::fill(info_out, info_out + APAP_MODEL_INFO, NAN);
    if (H_out) std::fill(H_out, H_out + 9, NAN);
    if (!pts_c || !pts_o || !weights || !params || !H_out || !info_out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    if (n < 1 || n > (1 << 26)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: n=%d (need 1 .. 2^26 matches)", who, n);
    HostCall call(ctx);
    int rc = call.select(device);
    if (rc) return rc;
    Layout io = call.layout(S_AUX);
    const Part pc = io.take((size_t)n * 2 * sizeof(float)), po = io.take((size_t)n * 2 * sizeof(float));
    const Part w = io.take((size_t)n * sizeof(float)), H = io.take(9 * sizeof(float)), info = io.take(APAP_MODEL_INFO * sizeof(double));
    call.alloc(io);
    const Part work = call.slot(S_WORK, apap_model_workspace_bytes(n));
    call.up(pc, pts_c);
    call.up(po, pts_o);
    call.up(w, weights);
    if ((rc = call.rc())) return rc;
    rc = apap_model_solve_device(ctx, pc.as<const float>(), po.as<const float>(), w.as<const float>(), n, params, H.as<float>(),
                                 info.as<double>(), nullptr, work.as<void>(), work.bytes, call.stream());
    if (rc) return rc;
    call.down(H_out, H);
    call.down(info_out, info);
    if ((rc = call.wait())) return rc;
    return model_status_code((int)info_out[APAP_MODEL_INFO_STATUS], who, 0);
}

int apap_spectral_em(apap_ctx *ctx, const float *src, const float *dst, const float *c_feats, const float *o_feats, int n,
                     const double *F, const double *spec_params, const double *model_params, int em_steps, const float *mask_in,
                     float *H_out, double *info_out, double *segment_out, float *ransac_mask_out, float *original_mask_out,
                     double *spec_info_out, int device) {
    const char *who = "apap_spectral_em";
    if (info_out && em_steps >= 1 && em_steps <= 64) std::fill(info_out, info_out + (size_t)em_steps * APAP_MODEL_INFO, NAN);
    if (H_out && em_steps >= 1 && em_steps <= 64) std::fill(H_out, H_out + (size_t)em_steps * 9, NAN);
    if (!src || !dst || !c_feats || !o_feats || !F || !spec_params || !model_params || !mask_in || !H_out || !info_out ||
        !segment_out || !ransac_mask_out || !original_mask_out || !spec_info_out)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    if (n < 1 || n > (1 << 26)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: n=%d (need 1 .. 2^26 matches)", who, n);
    if (em_steps < 1 || em_steps > 64) return apap::fail(APAP_ERR_INVALID_ARG, "%s: em_steps %d (1 .. 64)", who, em_steps);
    HostCall call(ctx);
    int rc = call.select(device);
    if (rc) return rc;
    // the parts of one spectral call (its single-round outputs stay unused), then the per-round outputs
    Layout io = call.layout(S_AUX);
    const SpecIo p = spec_io(io, n, false);
    const size_t k = (size_t)em_steps;
    const Part H = io.take(k * 9 * sizeof(float)), info = io.take(k * APAP_MODEL_INFO * sizeof(double));
    const Part seg = io.take(k * n * sizeof(double)), rm = io.take(k * n * sizeof(float)), om = io.take(k * n * sizeof(float));
    const Part sinfo = io.take(k * APAP_SPECTRAL_INFO * sizeof(double));
    call.alloc(io);
    const Part work = call.slot(S_WORK, apap_spectral_workspace_bytes(n) + apap_model_workspace_bytes(n));
    spec_upload(call, p, src, dst, c_feats, o_feats, F);
    call.up(p.mask, mask_in);
    if ((rc = call.rc())) return rc;
    rc = apap::spectral_em_run(ctx, p.src.as<const float>(), p.dst.as<const float>(), p.c.as<const float>(), p.o.as<const float>(), n,
                               p.F.as<const double>(), spec_params, model_params, em_steps, p.mask.as<const float>(), H.as<float>(),
                               info.as<double>(), seg.as<double>(), rm.as<float>(), om.as<float>(), sinfo.as<double>(), nullptr,
                               work.as<void>(), work.bytes, call.stream(), 1);
    if (rc) return rc;
    call.down(H_out, H);
    call.down(info_out, info);
    call.down(segment_out, seg);
    call.down(ransac_mask_out, rm);
    call.down(original_mask_out, om);
    call.down(spec_info_out, sinfo);
    if ((rc = call.wait())) return rc;
    for (int r = 0; r < em_steps; ++r)
        if ((rc = model_status_code((int)info_out[(size_t)r * APAP_MODEL_INFO + APAP_MODEL_INFO_STATUS], who, r))) return rc;
    return APAP_OK;
}

int apap_spectral_em_batch(apap_ctx *ctx, const float *src, const float *dst, const float *c_feats, const float *o_feats,
                           const double *F, const float *mask_in, const int *pair_offset, int n_pairs, const int *pair_of,
                           const double *spec_params, const double *model_params, int n_problems, int em_steps, float *H_out,
                           double *info_out, double *segment_out, float *ransac_mask_out, float *original_mask_out,
                           double *spec_info_out, int *status_out, int device) {
    const char *who = "apap_spectral_em_batch";
    if (!src || !dst || !c_feats || !o_feats || !F || !mask_in || !pair_offset || !pair_of || !spec_params || !model_params ||
        !H_out || !info_out || !segment_out || !ransac_mask_out || !original_mask_out || !spec_info_out)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    int rc = apap::spectral_em_batch_check(pair_offset, n_pairs, pair_of, spec_params, model_params, n_problems, em_steps, who);
    if (rc) return rc;
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    const size_t N = (size_t)(pair_offset[n_pairs] - pair_offset[0]), B = (size_t)n_problems, k = (size_t)em_steps;
    size_t M = 0;   // matches over the problems
    for (int b = 0; b < n_problems; ++b) M += (size_t)(pair_offset[pair_of[b] + 1] - pair_offset[pair_of[b]]);
    Layout io = call.layout(S_AUX);
    const size_t pts = N * 2 * sizeof(float), feats = N * APAP_SPECTRAL_DIM * sizeof(float);
    const Part d_src = io.take(pts), d_dst = io.take(pts), d_c = io.take(feats), d_o = io.take(feats);
    const Part d_F = io.take((size_t)n_pairs * 9 * sizeof(double)), d_mask = io.take(N * sizeof(float));
    const Part H = io.take(B * k * 9 * sizeof(float)), info = io.take(B * k * APAP_MODEL_INFO * sizeof(double));
    const Part seg = io.take(k * M * sizeof(double)), rm = io.take(k * M * sizeof(float)), om = io.take(k * M * sizeof(float));
    const Part sinfo = io.take(B * k * APAP_SPECTRAL_INFO * sizeof(double)), status = io.take(B * sizeof(int));
    call.alloc(io);
    const Part work = call.slot(S_WORK, apap_spectral_em_batch_workspace_bytes(pair_offset, n_pairs, pair_of, n_problems));
    const size_t first = (size_t)pair_offset[0];   // the device arrays start at the first pair
    const std::vector<int> rel = relative_offsets(pair_offset, n_pairs);
    call.up(d_src, src + first * 2);
    call.up(d_dst, dst + first * 2);
    call.up(d_c, c_feats + first * APAP_SPECTRAL_DIM);
    call.up(d_o, o_feats + first * APAP_SPECTRAL_DIM);
    call.up(d_F, F);
    call.up(d_mask, mask_in + first);
    call.zero(status);
    if ((rc = call.rc())) return rc;
    rc = apap::spectral_em_batch_run(ctx, d_src.as<const float>(), d_dst.as<const float>(), d_c.as<const float>(),
                                     d_o.as<const float>(), d_F.as<const double>(), d_mask.as<const float>(), rel.data(), n_pairs,
                                     pair_of, spec_params, model_params, n_problems, em_steps, H.as<float>(), info.as<double>(),
                                     seg.as<double>(), rm.as<float>(), om.as<float>(), sinfo.as<double>(), status.as<int>(),
                                     work.as<void>(), work.bytes, call.stream(), 1);
    if (rc) return rc;
    call.down(H_out, H);
    call.down(info_out, info);
    call.down(segment_out, seg);
    call.down(ransac_mask_out, rm);
    call.down(original_mask_out, om);
    call.down(spec_info_out, sinfo);
    if (status_out) call.down(status_out, status);
    return call.wait();   // a problem's status is its own: see status_out and the info blocks
}

// ------------------------------------------------------------------ robust moving DLT (apap_local_model.hip)
int apap_local_model_solve(apap_ctx *ctx, const float *pts_c, const float *pts_o, const float *match_weights, int n,
                           const double *vertices, int cells, double gamma, double sigma, const double *params, float *H_out,
                           double *info_out, int *status_out, int device) {
    const char *who = "apap_local_model_solve";
    if (cells >= 1 && cells <= APAP_LOCAL_MODEL_MAX_CELLS) {   // an early return leaves no stale result behind
        if (H_out) std::fill(H_out, H_out + (size_t)cells * 9, NAN);
        if (info_out) std::fill(info_out, info_out + (size_t)cells * APAP_MODEL_INFO, NAN);
        if (status_out) std::fill(status_out, status_out + cells, 0);
    }
    if (!pts_c || !pts_o || !vertices || !params || !H_out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    int rc = apap::local_model_check(n, cells, gamma, sigma, params, who);
    if (rc) return rc;
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    Layout io = call.layout(S_AUX);
    const size_t B = (size_t)cells, pts = (size_t)n * 2 * sizeof(float);
    const Part pc = io.take(pts), po = io.take(pts), mw = io.take(match_weights ? (size_t)n * sizeof(float) : 0);
    const Part H = io.take(B * 9 * sizeof(float)), info = io.take(info_out ? B * APAP_MODEL_INFO * sizeof(double) : 0);
    const Part status = io.take(B * sizeof(int));
    call.alloc(io);
    const Part vert = call.slot(S_VERT, B * 2 * sizeof(double));
    const Part work = call.slot(S_WORK, apap_local_model_workspace_bytes(n, cells));
    call.up(pc, pts_c);
    call.up(po, pts_o);
    if (match_weights) call.up(mw, match_weights);
    call.up(vert, vertices);
    call.zero(status);
    if ((rc = call.rc())) return rc;
    rc = apap_local_model_solve_device(ctx, pc.as<const float>(), po.as<const float>(), match_weights ? mw.as<const float>() : nullptr,
                                       n, vert.as<const double>(), cells, gamma, sigma, params, H.as<float>(),
                                       info_out ? info.as<double>() : nullptr, status.as<int>(), work.as<void>(), work.bytes,
                                       call.stream());
    if (rc) return rc;
    call.down(H_out, H);
    if (info_out) call.down(info_out, info);
    if (status_out) call.down(status_out, status);
    return call.wait();   // a cell's status is its own: see status_out and the info blocks
}

// ------------------------------------------------------------------ descriptor matching (apap_match.hip)
// What the host-buffer batch calls of the two matchers stage alike: the offsets relative to the first pair (the device arrays
// start there), the parts of the descriptors and of the four common outputs, their uploads and downloads.
struct MatchIo {
    size_t q0, t0, NQ, NT;
    std::vector<int> qrel, trel;
    Part d_q, d_t, d_idx, d_dist, d_idx2, d_dist2;
    MatchIo(Layout &io, const int *q_offset, const int *t_offset, int n_pairs, bool idx2, bool dist2)
        : q0((size_t)q_offset[0]), t0((size_t)t_offset[0]), NQ((size_t)q_offset[n_pairs] - q0), NT((size_t)t_offset[n_pairs] - t0),
          qrel(relative_offsets(q_offset, n_pairs)), trel(relative_offsets(t_offset, n_pairs)) {
        const size_t row = APAP_MATCH_DIM * sizeof(float);
        d_q = io.take(NQ * row), d_t = io.take(NT * row), d_idx = io.take(NQ * sizeof(int)), d_dist = io.take(NQ * sizeof(float));
        d_idx2 = io.take(idx2 ? NQ * sizeof(int) : 0), d_dist2 = io.take(dist2 ? NQ * sizeof(float) : 0);
    }
    void up(HostCall &call, const float *q, const float *t) const {
        call.up(d_q, q + q0 * APAP_MATCH_DIM);
        call.up(d_t, t + t0 * APAP_MATCH_DIM);
    }
    void down(HostCall &call, int *idx, float *dist, int *idx2, float *dist2) const {
        call.down(idx + q0, d_idx);
        call.down(dist + q0, d_dist);
        if (idx2) call.down(idx2 + q0, d_idx2);
        if (dist2) call.down(dist2 + q0, d_dist2);
    }
};

int apap_match_descriptors_batch(apap_ctx *ctx, const float *q, const float *t, const int *q_offset, const int *t_offset,
                                 int n_pairs, int *idx, float *dist, int *idx2, float *dist2, int device) {
    const char *who = "apap_match_descriptors_batch";
    if (!q || !t || !q_offset || !t_offset || !idx || !dist) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    int rc = apap::match_check(q_offset, t_offset, n_pairs, who);
    if (rc) return rc;
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    Layout io = call.layout(S_AUX);
    const MatchIo m(io, q_offset, t_offset, n_pairs, idx2, dist2);
    call.alloc(io);
    const Part work = call.slot(S_WORK, apap_match_batch_workspace_bytes(m.qrel.data(), m.trel.data(), n_pairs));
    m.up(call, q, t);
    if ((rc = call.rc())) return rc;
    rc = apap_match_descriptors_batch_device(ctx, m.d_q.as<const float>(), m.d_t.as<const float>(), m.qrel.data(), m.trel.data(),
                                             n_pairs, m.d_idx.as<int>(), m.d_dist.as<float>(), idx2 ? m.d_idx2.as<int>() : nullptr,
                                             dist2 ? m.d_dist2.as<float>() : nullptr, work.as<void>(), work.bytes, call.stream());
    if (rc) return rc;
    m.down(call, idx, dist, idx2, dist2);
    return call.wait();
}

int apap_match_descriptors(apap_ctx *ctx, const float *q, int nq, const float *t, int nt, int *idx, float *dist, int *idx2,
                           float *dist2, int device) {
    const int qo[2] = {0, nq}, to[2] = {0, nt};
    return apap_match_descriptors_batch(ctx, q, t, qo, to, 1, idx, dist, idx2, dist2, device);
}

// ------------------------------------------------------------------ guided descriptor matching (apap_match_guided.hip)
int apap_guided_records(apap_ctx *ctx, const float *pts, int n, const double *model, int what, double *rec_out, int device) {
    const char *who = "apap_guided_records";
    int rc = apap::guided_records_check(n, model, what, who);
    if (rc) return rc;
    if (!pts || !rec_out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    Layout io = call.layout(S_AUX);
    const Part d_pts = io.take((size_t)n * 2 * sizeof(float)), d_model = io.take(model ? 9 * sizeof(double) : 0);
    const Part d_rec = io.take((size_t)n * 3 * sizeof(double));
    call.alloc(io);
    call.up(d_pts, pts);
    if (model) call.up(d_model, model);
    if ((rc = call.rc())) return rc;
    rc = apap_guided_records_device(ctx, d_pts.as<const float>(), n, model ? d_model.as<const double>() : nullptr, what,
                                    d_rec.as<double>(), call.stream());
    if (rc) return rc;
    call.down(rec_out, d_rec);
    return call.wait();
}

int apap_match_guided_batch(apap_ctx *ctx, const double *rec_q, const double *rec_t, const float *q, const float *t,
                            const int *q_offset, const int *t_offset, int n_pairs, int kind, const double *r2, int *idx, float *dist,
                            int *idx2, float *dist2, int *count, int *ridx, float *rdist, int device) {
    const char *who = "apap_match_guided_batch";
    if (!rec_q || !rec_t || !q || !t || !q_offset || !t_offset || !r2 || !idx || !dist)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    if (!ridx != !rdist) return apap::fail(APAP_ERR_INVALID_ARG, "%s: ridx and rdist go together (both or neither)", who);
    int rc = apap::guided_check(q_offset, t_offset, n_pairs, kind, r2, who);
    if (rc) return rc;
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    Layout io = call.layout(S_AUX);
    const MatchIo m(io, q_offset, t_offset, n_pairs, idx2, dist2);
    const size_t NQ = m.NQ, NT = m.NT, rec = 3 * sizeof(double);
    const Part d_rq = io.take(NQ * rec), d_rt = io.take(NT * rec), d_count = io.take(count ? NQ * sizeof(int) : 0);
    const Part d_ridx = io.take(ridx ? NT * sizeof(int) : 0), d_rdist = io.take(ridx ? NT * sizeof(float) : 0);
    call.alloc(io);
    const Part work = call.slot(S_WORK, apap_match_guided_batch_workspace_bytes(m.qrel.data(), m.trel.data(), n_pairs));
    m.up(call, q, t);
    call.up(d_rq, rec_q + m.q0 * 3);
    call.up(d_rt, rec_t + m.t0 * 3);
    if ((rc = call.rc())) return rc;
    rc = apap_match_guided_batch_device(ctx, d_rq.as<const double>(), d_rt.as<const double>(), m.d_q.as<const float>(),
                                        m.d_t.as<const float>(), m.qrel.data(), m.trel.data(), n_pairs, kind, r2, m.d_idx.as<int>(),
                                        m.d_dist.as<float>(), idx2 ? m.d_idx2.as<int>() : nullptr,
                                        dist2 ? m.d_dist2.as<float>() : nullptr, count ? d_count.as<int>() : nullptr,
                                        ridx ? d_ridx.as<int>() : nullptr, ridx ? d_rdist.as<float>() : nullptr, work.as<void>(),
                                        work.bytes, call.stream());
    if (rc) return rc;
    m.down(call, idx, dist, idx2, dist2);
    if (count) call.down(count + m.q0, d_count);
    if (ridx) call.down(ridx + m.t0, d_ridx);
    if (ridx) call.down(rdist + m.t0, d_rdist);
    return call.wait();
}

int apap_match_guided(apap_ctx *ctx, const double *rec_q, const float *q, int nq, const double *rec_t, const float *t, int nt,
                      int kind, double r2, int *idx, float *dist, int *idx2, float *dist2, int *count, int *ridx, float *rdist,
                      int device) {
    const int qo[2] = {0, nq}, to[2] = {0, nt};
    return apap_match_guided_batch(ctx, rec_q, rec_t, q, t, qo, to, 1, kind, &r2, idx, dist, idx2, dist2, count, ridx, rdist, device);
}

// ------------------------------------------------------------------ descriptor extraction (apap_sift.hip)
int apap_sift_describe_batch(apap_ctx *ctx, const uint8_t *const *imgs, const int *heights, const int *widths, const int *channels,
                             int n_images, const float *pts, const int *pt_offset, float *out, int device) {
    const char *who = "apap_sift_describe_batch";
    if (!imgs || !pts || !out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    int rc = apap::sift_check(heights, widths, channels, n_images, pt_offset, who);
    if (rc) return rc;
    for (int m = 0; m < n_images; ++m)
        if (!imgs[m]) return apap::fail(APAP_ERR_INVALID_ARG, "%s: image %d: null pointer", who, m);
    const size_t k0 = (size_t)pt_offset[0], N = (size_t)pt_offset[n_images] - k0;   // the device arrays start at the first image
    for (size_t k = 0; k < 2 * N; ++k)
        if (!std::isfinite(pts[2 * k0 + k]))
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: keypoint %zu has a non-finite coordinate", who, k0 + k / 2);
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    const std::vector<int> rel = relative_offsets(pt_offset, n_images);
    const std::vector<Part> d_img = image_parts(call, heights, widths, channels, n_images);
    Layout io = call.layout(S_AUX);
    const Part d_pts = io.take(N * 2 * sizeof(float)), d_out = io.take(N * APAP_SIFT_DIM * sizeof(float));
    call.alloc(io);
    const Part work = call.slot(S_WORK, apap_sift_workspace_bytes(n_images));
    const std::vector<const uint8_t *> d_imgs = upload_images(call, d_img, imgs);
    call.up(d_pts, pts + 2 * k0);
    if ((rc = call.rc())) return rc;
    rc = apap_sift_describe_batch_device(ctx, d_imgs.data(), heights, widths, channels, n_images, d_pts.as<const float>(), rel.data(),
                                         d_out.as<float>(), work.as<void>(), work.bytes, call.stream());
    if (rc) return rc;
    call.down(out + k0 * APAP_SIFT_DIM, d_out);
    return call.wait();
}

int apap_sift_describe(apap_ctx *ctx, const uint8_t *img, int h, int w, int channels, const float *pts, int n, float *out, int device) {
    const int off[2] = {0, n};
    return apap_sift_describe_batch(ctx, &img, &h, &w, &channels, 1, pts, off, out, device);
}

// ------------------------------------------------------------------ keypoint orientation (apap_sift_orient.hip)
// The three host-buffer forms in one: angles out only (out null), descriptors at given angles (angles_in), or both.
static int sift_oriented_host(apap_ctx *ctx, const char *who, const uint8_t *const *imgs, const int *heights, const int *widths,
                              const int *channels, int n_images, const float *pts, const int *pt_offset, const float *angles_in,
                              float *angles_out, float *out, int device) {
    if (!imgs || !pts || (!angles_in && !angles_out)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    if (angles_in && angles_out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: angles are given: angles_out must be null", who);
    int rc = apap::sift_orient_check(heights, widths, channels, n_images, pt_offset, who);
    if (rc) return rc;
    for (int m = 0; m < n_images; ++m)
        if (!imgs[m]) return apap::fail(APAP_ERR_INVALID_ARG, "%s: image %d: null pointer", who, m);
    const size_t k0 = (size_t)pt_offset[0], N = (size_t)pt_offset[n_images] - k0;   // the device arrays start at the first image
    for (size_t k = 0; k < 2 * N; ++k)
        if (!std::isfinite(pts[2 * k0 + k]))
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: keypoint %zu has a non-finite coordinate", who, k0 + k / 2);
    for (size_t k = 0; angles_in && k < N; ++k)
        if (!(angles_in[k0 + k] >= 0.f && angles_in[k0 + k] <= 360.f))
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: keypoint %zu: angle %g is not in [0, 360]", who, k0 + k, (double)angles_in[k0 + k]);
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    const std::vector<int> rel = relative_offsets(pt_offset, n_images);
    const std::vector<Part> d_img = image_parts(call, heights, widths, channels, n_images);
    Layout io = call.layout(S_AUX);
    const Part d_pts = io.take(N * 2 * sizeof(float)), d_ang = io.take(N * sizeof(float));
    const Part d_out = io.take(out ? N * APAP_SIFT_DIM * sizeof(float) : 0);
    call.alloc(io);
    const Part work = call.slot(S_WORK, apap_sift_orient_workspace_bytes(n_images));
    const std::vector<const uint8_t *> d_imgs = upload_images(call, d_img, imgs);
    call.up(d_pts, pts + 2 * k0);
    if (angles_in) call.up(d_ang, angles_in + k0);
    if ((rc = call.rc())) return rc;
    const float *in = angles_in ? d_ang.as<const float>() : nullptr;
    float *ang_out = angles_in ? nullptr : d_ang.as<float>();
    if (out)
        rc = apap_sift_describe_oriented_batch_device(ctx, d_imgs.data(), heights, widths, channels, n_images, d_pts.as<const float>(),
                                                      rel.data(), in, ang_out, d_out.as<float>(), work.as<void>(), work.bytes, call.stream());
    else
        rc = apap_sift_orient_batch_device(ctx, d_imgs.data(), heights, widths, channels, n_images, d_pts.as<const float>(), rel.data(),
                                           ang_out, work.as<void>(), work.bytes, call.stream());
    if (rc) return rc;
    if (angles_out) call.down(angles_out + k0, d_ang);
    if (out) call.down(out + k0 * APAP_SIFT_DIM, d_out);
    return call.wait();
}

int apap_sift_orient_batch(apap_ctx *ctx, const uint8_t *const *imgs, const int *heights, const int *widths, const int *channels,
                           int n_images, const float *pts, const int *pt_offset, float *angles, int device) {
    return sift_oriented_host(ctx, "apap_sift_orient_batch", imgs, heights, widths, channels, n_images, pts, pt_offset, nullptr, angles,
                              nullptr, device);
}

int apap_sift_orient(apap_ctx *ctx, const uint8_t *img, int h, int w, int channels, const float *pts, int n, float *angles, int device) {
    const int off[2] = {0, n};
    return sift_oriented_host(ctx, "apap_sift_orient", &img, &h, &w, &channels, 1, pts, off, nullptr, angles, nullptr, device);
}

int apap_sift_describe_oriented_batch(apap_ctx *ctx, const uint8_t *const *imgs, const int *heights, const int *widths,
                                      const int *channels, int n_images, const float *pts, const int *pt_offset, const float *angles,
                                      float *angles_out, float *out, int device) {
    const char *who = "apap_sift_describe_oriented_batch";
    if (!out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    return sift_oriented_host(ctx, who, imgs, heights, widths, channels, n_images, pts, pt_offset, angles, angles_out, out, device);
}

int apap_sift_describe_oriented(apap_ctx *ctx, const uint8_t *img, int h, int w, int channels, const float *pts, int n,
                                const float *angles, float *angles_out, float *out, int device) {
    const char *who = "apap_sift_describe_oriented";
    if (!out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    const int off[2] = {0, n};
    return sift_oriented_host(ctx, who, &img, &h, &w, &channels, 1, pts, off, angles, angles_out, out, device);
}

// ------------------------------------------------------------------ corner detection (apap_corner.hip)
int apap_corner_detect_batch(apap_ctx *ctx, const uint8_t *const *imgs, const int *heights, const int *widths, const int *channels,
                             int n_images, int max_corners, int radius, int quality_permille, float *pts, long long *response,
                             int *count, int device) {
    const char *who = "apap_corner_detect_batch";
    if (!imgs || !pts || !response || !count) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    int rc = apap::corner_check(heights, widths, channels, n_images, max_corners, radius, quality_permille, who);
    if (rc) return rc;
    for (int m = 0; m < n_images; ++m)
        if (!imgs[m]) return apap::fail(APAP_ERR_INVALID_ARG, "%s: image %d: null pointer", who, m);
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    const size_t rows = (size_t)n_images * (size_t)max_corners;
    const std::vector<Part> d_img = image_parts(call, heights, widths, channels, n_images);
    Layout io = call.layout(S_AUX);
    const Part d_pts = io.take(rows * 2 * sizeof(float)), d_resp = io.take(rows * sizeof(long long));
    const Part d_count = io.take((size_t)n_images * sizeof(int));
    call.alloc(io);
    const Part work = call.slot(S_WORK, apap_corner_workspace_bytes(heights, widths, n_images, radius));
    const std::vector<const uint8_t *> d_imgs = upload_images(call, d_img, imgs);
    if ((rc = call.rc())) return rc;
    rc = apap_corner_detect_batch_device(ctx, d_imgs.data(), heights, widths, channels, n_images, max_corners, radius, quality_permille,
                                         d_pts.as<float>(), d_resp.as<long long>(), d_count.as<int>(), work.as<void>(), work.bytes,
                                         call.stream());
    if (rc) return rc;
    call.down(pts, d_pts);
    call.down(response, d_resp);
    call.down(count, d_count);
    return call.wait();
}

int apap_corner_detect(apap_ctx *ctx, const uint8_t *img, int h, int w, int channels, int max_corners, int radius,
                       int quality_permille, float *pts, long long *response, int *count, int device) {
    return apap_corner_detect_batch(ctx, &img, &h, &w, &channels, 1, max_corners, radius, quality_permille, pts, response, count, device);
}

// ------------------------------------------------------------------ image pyramid (apap_pyramid.hip)
int apap_pyramid_build_batch(apap_ctx *ctx, const uint8_t *const *imgs, const int *heights, const int *widths, const int *channels,
                             int n_images, int n_levels, int half_steps, uint8_t *levels, int device) {
    const char *who = "apap_pyramid_build_batch";
    if (!imgs || !levels) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    int rc = apap::pyramid_check(heights, widths, channels, n_images, n_levels, who);
    if (rc) return rc;
    for (int m = 0; m < n_images; ++m)
        if (!imgs[m]) return apap::fail(APAP_ERR_INVALID_ARG, "%s: image %d: null pointer", who, m);
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    // every level of every picture: its place in `levels` (and in the device buffer alike) and its bytes
    std::vector<size_t> at, bytes;
    size_t total = 0;
    for (int m = 0; m < n_images; ++m) {
        int lh[APAP_PYRAMID_MAX_LEVELS], lw[APAP_PYRAMID_MAX_LEVELS];
        long long off[APAP_PYRAMID_MAX_LEVELS + 1];
        const int n = apap_pyramid_layout(heights[m], widths[m], n_levels, half_steps, lh, lw, off, nullptr, nullptr);
        for (int l = 0; l < n; ++l) {
            at.push_back(total + (size_t)off[l]);
            bytes.push_back((size_t)lh[l] * lw[l]);
        }
        total += (size_t)off[n];
    }
    const std::vector<Part> d_img = image_parts(call, heights, widths, channels, n_images);
    const Part d_levels = call.slot(S_OUT, total);
    const Part work = call.slot(S_WORK, apap_pyramid_workspace_bytes(n_images, n_levels));
    const std::vector<const uint8_t *> d_imgs = upload_images(call, d_img, imgs);
    if ((rc = call.rc())) return rc;
    rc = apap_pyramid_build_batch_device(ctx, d_imgs.data(), heights, widths, channels, n_images, n_levels, half_steps,
                                         d_levels.as<uint8_t>(), d_levels.bytes, work.as<void>(), work.bytes, call.stream());
    if (rc) return rc;
    for (size_t k = 0; k < at.size(); ++k) call.down(levels + at[k], Part{d_levels.base, at[k], bytes[k]});   // the levels alone
    return call.wait();
}

int apap_pyramid_build(apap_ctx *ctx, const uint8_t *img, int h, int w, int channels, int n_levels, int half_steps, uint8_t *levels,
                       int device) {
    return apap_pyramid_build_batch(ctx, &img, &h, &w, &channels, 1, n_levels, half_steps, levels, device);
}

int apap_pyramid_keypoints(apap_ctx *ctx, const float *slab_pts, const long long *slab_response, int slab_rows, const int *counts,
                           const int *scale_num, const int *scale_shift, const int *level_index, int n_level_images, float *pts,
                           float *level_pts, int *level, long long *response, int *level_offset, int device) {
    const char *who = "apap_pyramid_keypoints";
    if (!slab_pts || !slab_response || !pts || !level_pts || !level || !response || !level_offset)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    int rc = apap::pyramid_keypoints_check(slab_rows, counts, scale_num, scale_shift, level_index, n_level_images, who);
    if (rc) return rc;
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    size_t N = 0;
    for (int m = 0; m < n_level_images; ++m) N += (size_t)counts[m];
    const size_t rows = (size_t)n_level_images * (size_t)slab_rows;
    Layout io = call.layout(S_AUX);
    const Part d_spts = io.take(rows * 2 * sizeof(float)), d_sresp = io.take(rows * sizeof(long long));
    const Part d_pts = io.take(N * 2 * sizeof(float)), d_lpts = io.take(N * 2 * sizeof(float));
    const Part d_level = io.take(N * sizeof(int)), d_resp = io.take(N * sizeof(long long));
    call.alloc(io);
    const Part work = call.slot(S_WORK, apap_pyramid_keypoints_workspace_bytes(n_level_images));
    call.up(d_spts, slab_pts);
    call.up(d_sresp, slab_response);
    if ((rc = call.rc())) return rc;
    rc = apap_pyramid_keypoints_device(ctx, d_spts.as<const float>(), d_sresp.as<const long long>(), slab_rows, counts, scale_num,
                                       scale_shift, level_index, n_level_images, d_pts.as<float>(), d_lpts.as<float>(), d_level.as<int>(),
                                       d_resp.as<long long>(), level_offset, work.as<void>(), work.bytes, call.stream());
    if (rc) return rc;
    if (N) {
        call.down(pts, d_pts);
        call.down(level_pts, d_lpts);
        call.down(level, d_level);
        call.down(response, d_resp);
    }
    return call.wait();
}

// ------------------------------------------------------------------ global warp and blend (apap_image_warp.hip)
int apap_image_warp_batch(apap_ctx *ctx, const uint8_t *const *bases, const int *base_h, const int *base_w, const uint8_t *const *srcs,
                          const int *src_h, const int *src_w, const double *M, const int *canvas_w, const int *canvas_h,
                          const int *off_x, const int *off_y, const int *direct_blend, int n_problems, uint8_t *out,
                          const long long *out_offset, int device) {
    const char *who = "apap_image_warp_batch";
    if (!bases || !srcs || !out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    int rc = apap::image_warp_check(base_h, base_w, src_h, src_w, M, canvas_w, canvas_h, off_x, off_y, direct_blend, n_problems, out_offset, who);
    if (rc) return rc;
    for (int p = 0; p < n_problems; ++p)
        if (!bases[p] || !srcs[p]) return apap::fail(APAP_ERR_INVALID_ARG, "%s: problem %d: null pointer", who, p);
    Pictures pics;   // of the batch
    std::vector<int> base_pic((size_t)n_problems), src_pic((size_t)n_problems);
    long long lo = out_offset[0], hi = 0;   // the device canvases start at the lowest offset
    for (int p = 0; p < n_problems; ++p) {
        base_pic[p] = pics.add(bases[p], (size_t)base_h[p] * base_w[p] * 3);
        src_pic[p] = pics.add(srcs[p], (size_t)src_h[p] * src_w[p] * 3);
        lo = std::min(lo, out_offset[p]);
        hi = std::max(hi, out_offset[p] + (long long)canvas_h[p] * canvas_w[p] * 3);
    }
    std::vector<long long> rel((size_t)n_problems);
    for (int p = 0; p < n_problems; ++p) rel[p] = out_offset[p] - lo;
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    Layout imgs = call.layout(S_IMG);
    pics.take(imgs);
    call.alloc(imgs);
    const Part d_out = call.slot(S_OUT, (size_t)(hi - lo));
    const Part work = call.slot(S_WORK, apap_image_warp_workspace_bytes(n_problems));
    pics.upload(call);
    if ((rc = call.rc())) return rc;
    std::vector<const uint8_t *> d_bases((size_t)n_problems), d_srcs((size_t)n_problems);
    for (int p = 0; p < n_problems; ++p) {
        d_bases[p] = pics.dev(base_pic[p]);
        d_srcs[p] = pics.dev(src_pic[p]);
    }
    rc = apap_image_warp_batch_device(ctx, d_bases.data(), base_h, base_w, d_srcs.data(), src_h, src_w, M, canvas_w, canvas_h, off_x, off_y,
                                      direct_blend, n_problems, d_out.as<uint8_t>(), rel.data(), work.as<void>(), work.bytes, nullptr,
                                      call.stream());
    if (rc) return rc;
    for (int p = 0; p < n_problems; ++p)   // the bytes between the canvases are not the call's
        call.down(out + out_offset[p], Part{d_out.base, (size_t)rel[p], (size_t)canvas_h[p] * canvas_w[p] * 3});
    return call.wait();
}

int apap_image_warp(apap_ctx *ctx, const uint8_t *base, int h1, int w1, const uint8_t *src, int h2, int w2, const double *M,
                    int canvas_w, int canvas_h, int off_x, int off_y, int direct_blend, uint8_t *out, int device) {
    const long long at = 0;
    return apap_image_warp_batch(ctx, &base, &h1, &w1, &src, &h2, &w2, M, &canvas_w, &canvas_h, &off_x, &off_y, &direct_blend, 1, out, &at,
                                 device);
}

// ------------------------------------------------------------------ panorama (apap_panorama.hip)
// `status` (may be NULL) receives the n_layers status words whatever the call returns once the kernels ran.  `ramp` as in
// apap::panorama_check: NULL for apap_panorama, the ramp width for apap_panorama_ramp.  `gain` (NULL: the plain blend): what the
// gain entry points ask for - the blend under gain_q (kPanoGain), the statistics alone (kPanoStats, no `out`), or statistics,
// the solve on the host and the blend under its gains (kPanoAuto: two passes, each with the layers' set-up).  `band` (NULL for
// every other blend): the two-band blend's radius; its workspace holds the views' low-pass pictures too.
struct HostGain {
    int what;
    const int *gain_q;
    int step;
    double sigma_n, sigma_g;
    unsigned long long *N, *S;
    double *g;
    int *q, *flag;
};
static int panorama_host(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs, const int *img_h,
                  const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols, const double *const *mesh_w,
                  const int *n_w, const double *const *mesh_h, const int *n_h, const int *final_w, const int *final_h, const int *off_x,
                  const int *off_y, int n_layers, int mode, const int *ramp, uint8_t *out, int *status, int device, const char *who,
                  const HostGain *gain = nullptr, const int *band = nullptr) {
    int b[4];
    int rc = band ? apap::panorama_band_check(*band, who) : APAP_OK;
    if (rc) return rc;
    rc = apap::panorama_check(center_h, center_w, img_h, img_w, mesh_rows, mesh_cols, n_w, n_h, final_w, final_h, off_x, off_y,
                                  n_layers, mode, ramp, b, who);
    if (rc) return rc;
    const int what = gain ? gain->what : apap::kPanoPlain;
    const bool stats = what == apap::kPanoStats || what == apap::kPanoAuto, blend = what != apap::kPanoStats;
    if (gain) {
        const bool solve = what == apap::kPanoAuto;
        if ((rc = apap::panorama_gain_check(n_layers + 1, stats ? &gain->step : nullptr, what == apap::kPanoGain ? gain->gain_q : nullptr,
                                            solve ? &gain->sigma_n : nullptr, solve ? &gain->sigma_g : nullptr, who)))
            return rc;
        if ((what == apap::kPanoGain && !gain->gain_q) || (stats && (!gain->N || !gain->S)) || (solve && (!gain->g || !gain->q || !gain->flag)))
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    }
    if (!center || !imgs || !Hfwd || !mesh_w || !mesh_h || (blend && !out)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    for (int k = 0; k < n_layers; ++k)
        if (!imgs[k] || !Hfwd[k] || !mesh_w[k] || !mesh_h[k]) return apap::fail(APAP_ERR_INVALID_ARG, "%s: layer %d: null pointer", who, k);
    // picture 0 is the centre, on its own: only the layers share pictures, among themselves
    Pictures pics;
    pics.add(center, (size_t)center_h * center_w * 3, false);
    std::vector<int> pic_of((size_t)n_layers);
    for (int k = 0; k < n_layers; ++k) pic_of[k] = pics.add(imgs[k], (size_t)img_h[k] * img_w[k] * 3);
    std::vector<int> st((size_t)n_layers, 0);       // before the HostCall: a download writes it
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    Layout l_img = call.layout(S_IMG), l_h = call.layout(S_H), l_mw = call.layout(S_MESHW), l_mh = call.layout(S_MESHH);
    std::vector<Part> d_h((size_t)n_layers, Part{}), d_mw((size_t)n_layers, Part{}), d_mh((size_t)n_layers, Part{});
    pics.take(l_img);
    for (int k = 0; k < n_layers; ++k) {
        d_h[k] = l_h.take((size_t)mesh_rows[k] * mesh_cols[k] * 9 * sizeof(float));
        d_mw[k] = l_mw.take((size_t)n_w[k] * sizeof(double));
        d_mh[k] = l_mh.take((size_t)n_h[k] * sizeof(double));
    }
    call.alloc(l_img); call.alloc(l_h); call.alloc(l_mw); call.alloc(l_mh);
    const Part d_out = blend ? call.slot(S_OUT, (size_t)b[0] * b[1] * 3) : Part{};
    const Part d_status = call.slot(S_STATUS, (size_t)n_layers * sizeof(int));
    const Part work = call.slot(S_WORK, band ? apap_panorama_band_workspace_bytes(center_h, center_w, img_h, img_w, mesh_rows, mesh_cols, final_w,
                                                                                  final_h, n_layers, *band)
                                             : apap_panorama_workspace_bytes(mesh_rows, mesh_cols, final_w, final_h, n_layers));
    const size_t table_bytes = (size_t)(n_layers + 1) * (n_layers + 1) * sizeof(unsigned long long);
    Layout l_tab = call.layout(S_AUX);
    const Part d_N = l_tab.take(stats ? table_bytes : 0), d_S = l_tab.take(stats ? table_bytes : 0);
    if (stats) call.alloc(l_tab);
    pics.upload(call);
    for (int k = 0; k < n_layers; ++k) {
        call.up(d_h[k], Hfwd[k]);
        call.up(d_mw[k], mesh_w[k]);
        call.up(d_mh[k], mesh_h[k]);
    }
    call.zero(d_status);
    if ((rc = call.rc())) return rc;
    std::vector<const uint8_t *> p_img((size_t)n_layers);
    std::vector<const float *> p_h((size_t)n_layers);
    std::vector<const double *> p_mw((size_t)n_layers), p_mh((size_t)n_layers);
    for (int k = 0; k < n_layers; ++k) {
        p_img[k] = pics.dev(pic_of[k]);
        p_h[k] = d_h[k].as<const float>();
        p_mw[k] = d_mw[k].as<const double>();
        p_mh[k] = d_mh[k].as<const double>();
    }
    const apap::PanoGeometry G{pics.dev(0), center_h, center_w, p_img.data(), img_h, img_w, p_h.data(), mesh_rows, mesh_cols, p_mw.data(),
                               n_w, p_mh.data(), n_h, final_w, final_h, off_x, off_y, n_layers};
    apap::PanoJob J;
    J.mode = mode; J.ramp = ramp; J.band = band;
    if (stats) {
        J.what = apap::kPanoStats;
        J.step = gain->step; J.d_N = d_N.as<unsigned long long>(); J.d_S = d_S.as<unsigned long long>();
        if ((rc = apap::panorama_run(ctx, G, J, work.as<void>(), work.bytes, d_status.as<int>(), call.stream(), who))) return rc;
        call.down(gain->N, d_N);
        call.down(gain->S, d_S);
        if (blend) {    // the solve on the host, between the two passes
            if ((rc = call.wait())) return rc;
            *gain->flag = apap::panorama_gain_solve_host(gain->N, gain->S, n_layers + 1, gain->sigma_n, gain->sigma_g, gain->g, gain->q);
        }
    }
    if (blend) {
        J.what = gain ? apap::kPanoGain : apap::kPanoPlain;
        J.gain_q = !gain ? nullptr : what == apap::kPanoAuto ? gain->q : gain->gain_q;
        J.d_out = d_out.as<uint8_t>();
        if ((rc = apap::panorama_run(ctx, G, J, work.as<void>(), work.bytes, d_status.as<int>(), call.stream(), who))) return rc;
        call.down(out, d_out);
    }
    call.down(st.data(), d_status);
    if ((rc = call.wait())) return rc;
    if (status) std::copy(st.begin(), st.end(), status);
    for (int k = 0; k < n_layers; ++k) {
        char layer[48];
        snprintf(layer, sizeof(layer), "%s: layer %d", who, k);
        if ((rc = status_to_code(st[k], layer))) return rc;
    }
    return APAP_OK;
}

int apap_panorama(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs, const int *img_h,
                  const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols, const double *const *mesh_w,
                  const int *n_w, const double *const *mesh_h, const int *n_h, const int *final_w, const int *final_h, const int *off_x,
                  const int *off_y, int n_layers, int mode, uint8_t *out, int *status, int device) {
    return panorama_host(ctx, center, center_h, center_w, imgs, img_h, img_w, Hfwd, mesh_rows, mesh_cols, mesh_w, n_w, mesh_h, n_h, final_w,
                         final_h, off_x, off_y, n_layers, mode, nullptr, out, status, device, "apap_panorama");
}

int apap_panorama_ramp(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs, const int *img_h,
                       const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols,
                       const double *const *mesh_w, const int *n_w, const double *const *mesh_h, const int *n_h, const int *final_w,
                       const int *final_h, const int *off_x, const int *off_y, int n_layers, int ramp, uint8_t *out, int *status,
                       int device) {
    return panorama_host(ctx, center, center_h, center_w, imgs, img_h, img_w, Hfwd, mesh_rows, mesh_cols, mesh_w, n_w, mesh_h, n_h, final_w,
                         final_h, off_x, off_y, n_layers, APAP_PANORAMA_RAMP, &ramp, out, status, device, "apap_panorama_ramp");
}

int apap_panorama_gain_stats(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs,
                             const int *img_h, const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols,
                             const double *const *mesh_w, const int *n_w, const double *const *mesh_h, const int *n_h,
                             const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers, int step,
                             unsigned long long *N, unsigned long long *S, int *status, int device) {
    const HostGain g{apap::kPanoStats, nullptr, step, 0.0, 0.0, N, S, nullptr, nullptr, nullptr};
    return panorama_host(ctx, center, center_h, center_w, imgs, img_h, img_w, Hfwd, mesh_rows, mesh_cols, mesh_w, n_w, mesh_h, n_h, final_w,
                         final_h, off_x, off_y, n_layers, APAP_PANORAMA_MEAN, nullptr, nullptr, status, device, "apap_panorama_gain_stats", &g);
}

int apap_panorama_gain(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs, const int *img_h,
                       const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols,
                       const double *const *mesh_w, const int *n_w, const double *const *mesh_h, const int *n_h, const int *final_w,
                       const int *final_h, const int *off_x, const int *off_y, int n_layers, int mode, int ramp, const int *gain_q,
                       uint8_t *out, int *status, int device) {
    const HostGain g{apap::kPanoGain, gain_q, 1, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr};
    return panorama_host(ctx, center, center_h, center_w, imgs, img_h, img_w, Hfwd, mesh_rows, mesh_cols, mesh_w, n_w, mesh_h, n_h, final_w,
                         final_h, off_x, off_y, n_layers, mode, mode == APAP_PANORAMA_RAMP ? &ramp : nullptr, out, status, device,
                         "apap_panorama_gain", &g);
}

int apap_panorama_auto_gain(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs,
                            const int *img_h, const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols,
                            const double *const *mesh_w, const int *n_w, const double *const *mesh_h, const int *n_h,
                            const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers, int mode, int ramp,
                            int step, double sigma_n, double sigma_g, uint8_t *out, unsigned long long *N, unsigned long long *S,
                            double *g, int *q, int *flag, int *status, int device) {
    const HostGain hg{apap::kPanoAuto, nullptr, step, sigma_n, sigma_g, N, S, g, q, flag};
    return panorama_host(ctx, center, center_h, center_w, imgs, img_h, img_w, Hfwd, mesh_rows, mesh_cols, mesh_w, n_w, mesh_h, n_h, final_w,
                         final_h, off_x, off_y, n_layers, mode, mode == APAP_PANORAMA_RAMP ? &ramp : nullptr, out, status, device,
                         "apap_panorama_auto_gain", &hg);
}

int apap_panorama_band(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs, const int *img_h,
                       const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols,
                       const double *const *mesh_w, const int *n_w, const double *const *mesh_h, const int *n_h, const int *final_w,
                       const int *final_h, const int *off_x, const int *off_y, int n_layers, int ramp, int band, const int *gain_q,
                       uint8_t *out, int *status, int device) {
    const HostGain g{apap::kPanoGain, gain_q, 1, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr};
    return panorama_host(ctx, center, center_h, center_w, imgs, img_h, img_w, Hfwd, mesh_rows, mesh_cols, mesh_w, n_w, mesh_h, n_h, final_w,
                         final_h, off_x, off_y, n_layers, APAP_PANORAMA_BAND, &ramp, out, status, device, "apap_panorama_band",
                         gain_q ? &g : nullptr, &band);
}

int apap_box_blur(apap_ctx *ctx, const uint8_t *img, int h, int w, int radius, uint8_t *out, int device) {
    const char *who = "apap_box_blur";
    int rc = apap::box_blur_check(h, w, radius, who);
    if (rc) return rc;
    if (!img || !out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    const size_t bytes = (size_t)h * w * 3;
    HostCall call(ctx);
    if ((rc = call.select(device))) return rc;
    const Part d_img = call.slot(S_IMG, bytes), d_out = call.slot(S_OUT, bytes);
    call.up(d_img, img);
    if ((rc = call.rc())) return rc;
    if ((rc = apap_box_blur_device(ctx, d_img.as<const uint8_t>(), h, w, radius, d_out.as<uint8_t>(), call.stream()))) return rc;
    call.down(out, d_out);
    return call.wait();
}

}  // extern "C"
