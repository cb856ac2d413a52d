// orbfe_pool.cpp -- the multi-device pool (orbfe.h: "Multi-device pool"): N handles with one ring each, the frames of a
// call sharded over them in contiguous blocks, every member driving its own ring on a worker thread of its own.
//
// No device work of its own: per frame the members enqueue exactly the chain orbfe_stream_submit / _submit_track enqueue
// (upload, extraction, optionally isInFrustum + SearchByProjection, download), which is what keeps the results
// byte-identical to the single-handle calls.  What lives here is the host side: the shard arithmetic, the workers, the
// argument checks made once on the calling thread, and the drain after a failure.
#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "match.h"

namespace {

constexpr int kMaxMembers = 16;

struct Member {
    orbfe_handle* h = nullptr;
    orbfe_stream* st = nullptr;
    orbfe_map* map = nullptr;
    int device = 0;
    long long frames = 0;             // collected since create
    int rc = ORBFE_OK;                // status of the member's part of the current call
    std::vector<int> inFlight;        // first frame of every uncollected submission, oldest first (a ring of nSlots)
    std::thread worker;
};

}  // namespace

struct orbfe_pool {
    std::vector<Member> m;
    int nSlots = 0, slotFrames = 0;
    int width = 0, height = 0, nLevels = 0, cap = 0;
    int mapCap = 0, maxPoints = 0;  // 0: orbfe_pool_enable_track not yet made
    std::string err;
    // one job at a time: the caller publishes it under `mu` and bumps `gen`; every worker runs job(k) once per generation
    std::mutex mu;
    std::condition_variable cvWork, cvDone;
    const std::function<int(int)>* job = nullptr;
    unsigned long long gen = 0;
    int pending = 0;
    bool stop = false;
    bool busy = false;  // a pool call is running (one caller at a time; the flag turns a second one away)
};

namespace {

void worker_loop(orbfe_pool* p, int k)
{
    unsigned long long seen = 0;
    for (;;) {
        const std::function<int(int)>* fn;
        {
            std::unique_lock<std::mutex> lk(p->mu);
            p->cvWork.wait(lk, [&] { return p->stop || p->gen != seen; });
            if (p->stop) return;
            seen = p->gen;
            fn = p->job;
        }
        const int rc = (*fn)(k);
        std::lock_guard<std::mutex> lk(p->mu);
        p->m[(size_t)k].rc = rc;
        if (--p->pending == 0) p->cvDone.notify_all();
    }
}

// runs fn(k) on every member's worker at the same time and waits (asleep) for all of them; the status of the
// lowest-numbered failing member, with its handle's message in p->err
int run_members(orbfe_pool* p, const std::function<int(int)>& fn)
{
    {
        std::lock_guard<std::mutex> lk(p->mu);
        p->job = &fn;
        p->pending = (int)p->m.size();
        p->gen++;
    }
    p->cvWork.notify_all();
    {
        std::unique_lock<std::mutex> lk(p->mu);
        p->cvDone.wait(lk, [&] { return p->pending == 0; });
        p->job = nullptr;
    }
    for (size_t k = 0; k < p->m.size(); k++) {
        const Member& mb = p->m[k];
        if (mb.rc != ORBFE_OK) {
            char buf[64];
            snprintf(buf, sizeof buf, "member %d (device %d): ", (int)k, mb.device);
            p->err = std::string(buf) + orbfe_last_error(mb.h);
            return mb.rc;
        }
    }
    return ORBFE_OK;
}

// marks the pool busy for the duration of one call; a second concurrent caller is refused
struct BusyScope {
    orbfe_pool* p;
    bool ok;
    explicit BusyScope(orbfe_pool* p_) : p(p_)
    {
        std::lock_guard<std::mutex> lk(p->mu);
        ok = !p->busy;
        p->busy = true;
    }
    ~BusyScope()
    {
        if (!ok) return;
        std::lock_guard<std::mutex> lk(p->mu);
        p->busy = false;
    }
};

void release_members(orbfe_pool* p)
{
    {
        std::lock_guard<std::mutex> lk(p->mu);
        p->stop = true;
    }
    p->cvWork.notify_all();
    for (auto& mb : p->m)
        if (mb.worker.joinable()) mb.worker.join();
    // ring, then map (it detaches from the ring that is already gone), then the handle that owns both
    for (auto& mb : p->m) {
        orbfe_stream_destroy(mb.st);
        orbfe_map_destroy(mb.map);
        orbfe_destroy(mb.h);
        mb.st = nullptr;
        mb.map = nullptr;
        mb.h = nullptr;
    }
}

struct Outputs {
    orbfe_keypoint* kp;
    uint8_t* desc;
    int* n;
    int* per;
    int* match;     // track only
    int* nMatches;  // track only
};

struct TrackArgs {
    const orbfe_track_params* tp;
    const orbfe_frustum* frusta;
    int nPoints;
    const int* ids;
};

// member k's share of one call: its block through its ring, `slots` submissions in flight, each collected straight into the
// caller's arrays at the absolute offset of its first frame.  On a failure nothing more is submitted and everything in
// flight is waited for and dropped.
int member_run(orbfe_pool* p, int k, const uint8_t* const* grays, int pitch, int nFrames, const Outputs& o, const TrackArgs* t)
{
    Member& mb = p->m[(size_t)k];
    int lo = 0, hi = 0;
    orbfe_shard_range(nFrames, k, (int)p->m.size(), &lo, &hi);
    const size_t cap = (size_t)p->cap;
    const int nL = p->nLevels;
    int head = 0, count = 0;  // mb.inFlight[head .. head + count) (mod nSlots)
    auto collect = [&]() {
        const int off = mb.inFlight[(size_t)head];
        int nf = 0;
        const int rc = t ? orbfe_stream_collect_track(mb.st, o.kp + off * cap, o.desc + off * cap * ORBFE_DESC_BYTES, o.n + off,
                                                      o.per ? o.per + (size_t)off * nL : nullptr, o.match + off * cap, o.nMatches + off, &nf)
                         : orbfe_stream_collect(mb.st, o.kp + off * cap, o.desc + off * cap * ORBFE_DESC_BYTES, o.n + off,
                                                o.per ? o.per + (size_t)off * nL : nullptr, &nf);
        head = (head + 1) % p->nSlots;
        count--;
        if (rc == ORBFE_OK) mb.frames += nf;
        return rc;
    };
    int rc = ORBFE_OK;
    for (int i = lo; i < hi && rc == ORBFE_OK;) {
        if (count == p->nSlots) {  // ring full: the oldest submission first (the ring never answers ORBFE_ERR_BUSY here)
            rc = collect();
            continue;
        }
        const int n = std::min(p->slotFrames, hi - i);
        rc = t ? orbfe_stream_submit_track(mb.st, grays + i, pitch, n, t->tp, t->frusta + i, t->nPoints,
                                           t->ids ? t->ids + (size_t)i * t->nPoints : nullptr)
               : orbfe_stream_submit(mb.st, grays + i, pitch, n);
        if (rc != ORBFE_OK) break;
        mb.inFlight[(size_t)((head + count) % p->nSlots)] = i;
        count++;
        i += n;
    }
    while (rc == ORBFE_OK && count > 0) rc = collect();
    if (rc != ORBFE_OK) orbfe_stream_drain(mb.st);  // (a failed collect may have left its submission in flight)
    return rc;
}

// the checks stream_submit_impl makes per submission, made once for the whole call on the calling thread
int check_frames(const orbfe_pool* p, const uint8_t* const* grays, int pitch, int nFrames, const Outputs& o)
{
    if (!grays || !o.kp || !o.desc || !o.n || nFrames < 1) return ORBFE_ERR_INVALID_ARG;
    if (pitch < p->width || pitch >= (1 << 24)) return ORBFE_ERR_INVALID_ARG;
    if ((size_t)pitch * (p->height - 1) + (size_t)((p->width + 3) & ~3) >= (size_t)0x7ffffff0u) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < nFrames; i++)
        if (!grays[i]) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

}  // namespace

extern "C" {

int orbfe_shard_range(int n_frames, int k, int n_members, int* lo, int* hi)
{
    if (!lo || !hi || n_frames < 0 || n_members < 1 || k < 0 || k >= n_members) return ORBFE_ERR_INVALID_ARG;
    const long long per = ((long long)n_frames + n_members - 1) / n_members;
    const long long l = std::min((long long)k * per, (long long)n_frames);
    *lo = (int)l;
    *hi = (int)std::min(l + per, (long long)n_frames);
    return ORBFE_OK;
}

int orbfe_pool_create(const orbfe_params* params, const int* devices, int n_devices, int slots, int slot_frames, orbfe_pool** out)
{
    if (!params || !devices || !out || n_devices < 1 || n_devices > kMaxMembers || slots < 2 || slots > 64 || slot_frames < 1 ||
        slot_frames > params->max_batch)
        return ORBFE_ERR_INVALID_ARG;
    *out = nullptr;
    for (int k = 0; k < n_devices; k++)
        if (devices[k] < 0) return ORBFE_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return ORBFE_ERR_NO_DEVICE;
    }
    for (int k = 0; k < n_devices; k++)
        if (devices[k] >= ndev) return ORBFE_ERR_INVALID_ARG;

    orbfe_pool* p = new (std::nothrow) orbfe_pool();
    if (!p) return ORBFE_ERR_OUT_OF_MEMORY;
    p->nSlots = slots;
    p->slotFrames = slot_frames;
    p->width = params->image_width;
    p->height = params->image_height;
    p->nLevels = params->n_levels;
    int rc = ORBFE_OK;
    try {
        p->m.resize((size_t)n_devices);
        // a ring's copy pool defaults to min(7, cores / 2) threads: the members share that budget instead of multiplying it
        const int copyThreads = std::max(1, 7 / n_devices);
        for (int k = 0; k < n_devices && rc == ORBFE_OK; k++) {
            Member& mb = p->m[(size_t)k];
            orbfe_params prm = *params;
            prm.device_id = devices[k];
            mb.device = devices[k];
            mb.inFlight.assign((size_t)slots, 0);
            rc = orbfe_create(&prm, &mb.h);
            if (rc == ORBFE_OK) rc = orbfe_stream_create_copy_threads(mb.h, slots, slot_frames, copyThreads, &mb.st);
        }
        if (rc == ORBFE_OK) {
            p->cap = orbfe_max_keypoints(p->m[0].h);
            for (int k = 0; k < n_devices; k++) p->m[(size_t)k].worker = std::thread(worker_loop, p, k);
        }
    } catch (const std::bad_alloc&) {
        rc = ORBFE_ERR_OUT_OF_MEMORY;
    } catch (const std::system_error&) {  // a worker thread could not be started
        rc = ORBFE_ERR_OUT_OF_MEMORY;
    }
    if (rc != ORBFE_OK) {
        release_members(p);
        delete p;
        return rc;
    }
    *out = p;
    return ORBFE_OK;
}

void orbfe_pool_destroy(orbfe_pool* p)
{
    if (!p) return;
    release_members(p);
    delete p;
}

int orbfe_pool_size(const orbfe_pool* p) { return p ? (int)p->m.size() : 0; }

orbfe_handle* orbfe_pool_member(const orbfe_pool* p, int k)
{
    return p && k >= 0 && k < (int)p->m.size() ? p->m[(size_t)k].h : nullptr;
}

long long orbfe_pool_member_frames(const orbfe_pool* p, int k)
{
    return p && k >= 0 && k < (int)p->m.size() ? p->m[(size_t)k].frames : 0;
}

const char* orbfe_pool_last_error(const orbfe_pool* p) { return p ? p->err.c_str() : ""; }

int orbfe_pool_extract(orbfe_pool* p, const uint8_t* const* grays, int pitch, int n_frames, orbfe_keypoint* kp_out, uint8_t* desc_out,
                       int* n_out, int* per_level_counts)
{
    if (!p) return ORBFE_ERR_INVALID_ARG;
    const Outputs o{kp_out, desc_out, n_out, per_level_counts, nullptr, nullptr};
    const int rc = check_frames(p, grays, pitch, n_frames, o);
    if (rc != ORBFE_OK) return rc;
    BusyScope busy(p);
    if (!busy.ok) return ORBFE_ERR_INVALID_ARG;
    const std::function<int(int)> fn = [&](int k) { return member_run(p, k, grays, pitch, n_frames, o, nullptr); };
    return run_members(p, fn);
}

int orbfe_pool_enable_track(orbfe_pool* p, int map_capacity, int max_points)
{
    if (!p || map_capacity < 1 || map_capacity > (1 << 26) || max_points < 1 || max_points > (1 << 24)) return ORBFE_ERR_INVALID_ARG;
    BusyScope busy(p);
    if (!busy.ok || p->maxPoints != 0) return ORBFE_ERR_INVALID_ARG;
    int rc = ORBFE_OK;
    size_t k = 0;
    for (; k < p->m.size() && rc == ORBFE_OK; k++) {
        Member& mb = p->m[k];
        rc = orbfe_map_create(mb.h, map_capacity, &mb.map);
        if (rc == ORBFE_OK) rc = orbfe_stream_enable_track(mb.st, mb.map, max_points);
        if (rc != ORBFE_OK) {
            char buf[64];
            snprintf(buf, sizeof buf, "member %d (device %d): ", (int)k, mb.device);
            p->err = std::string(buf) + orbfe_last_error(mb.h);
        }
    }
    if (rc != ORBFE_OK) {  // give back what this call made on every member it reached: the pool is as it was
        for (size_t j = 0; j < k; j++) {
            Member& mb = p->m[j];
            orbfe_stream_release_track(mb.st);
            orbfe_map_destroy(mb.map);
            mb.map = nullptr;
        }
        return rc;
    }
    p->mapCap = map_capacity;
    p->maxPoints = max_points;
    return ORBFE_OK;
}

int orbfe_pool_map_update(orbfe_pool* p, int n, const int* ids, const orbfe_world_point* points, const uint8_t* desc)
{
    if (!p || p->maxPoints == 0 || n < 0 || (n > 0 && (!ids || !points || !desc))) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= p->mapCap) return ORBFE_ERR_INVALID_ARG;
    if (n == 0) return ORBFE_OK;
    BusyScope busy(p);
    if (!busy.ok) return ORBFE_ERR_INVALID_ARG;
    const std::function<int(int)> fn = [&](int k) {
        const Member& mb = p->m[(size_t)k];
        return orbfe_map_update(mb.h, mb.map, n, ids, points, desc);
    };
    return run_members(p, fn);
}

int orbfe_pool_track(orbfe_pool* p, const uint8_t* const* grays, int pitch, int n_frames, const orbfe_track_params* tp,
                     const orbfe_frustum* frusta, int n_points, const int* ids, orbfe_keypoint* kp_out, uint8_t* desc_out, int* n_out,
                     int* per_level_counts, int* match_out, int* n_matches)
{
    if (!p || !tp || !frusta || !match_out || !n_matches || p->maxPoints == 0) return ORBFE_ERR_INVALID_ARG;
    const Outputs o{kp_out, desc_out, n_out, per_level_counts, match_out, n_matches};
    int rc = check_frames(p, grays, pitch, n_frames, o);
    if (rc != ORBFE_OK) return rc;
    if (n_points < 0 || n_points > p->maxPoints || (n_points > 0 && !ids)) return ORBFE_ERR_INVALID_ARG;
    if (tp->struct_size != (int)sizeof(orbfe_track_params) || tp->grid_cols < 1 || tp->grid_rows < 1) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < n_frames; i++) {
        rc = orbfe::frustum_validate(&frusta[i]);
        if (rc != ORBFE_OK) return rc;
        if (frusta[i].n_levels > p->nLevels) return ORBFE_ERR_INVALID_ARG;
    }
    BusyScope busy(p);
    if (!busy.ok) return ORBFE_ERR_INVALID_ARG;
    const TrackArgs t{tp, frusta, n_points, n_points > 0 ? ids : nullptr};
    const std::function<int(int)> fn = [&](int k) { return member_run(p, k, grays, pitch, n_frames, o, &t); };
    return run_members(p, fn);
}

}  // extern "C"
