// staging.h -- the layout of one host-pointer call in the two grow-only arenas (device, pinned host).  Host-pure: no HIP header, so the
// layout is exercised without a GPU (tests/cpp/staging_layout.cpp).  reserve / upload / download are in match_common.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace orbfe {

// device offsets in take order, 256-byte granules
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off = (off + bytes + 255) / 256 * 256; return o; }
};

// one array of a call: where it lies on the device and how many T it holds
template <class T>
struct Block {
    size_t off = 0, n = 0;
    size_t bytes() const { return n * sizeof(T); }
    size_t end() const { return off + bytes(); }
};

// A call takes its blocks once, in three phases and in this order: in() -- filled on the host, [0, inBytes) goes up in one copy;
// scratch() -- device only; out() -- [oRes, oRes + resBytes) comes down in one span (or in pieces, download_span).  inout() is the
// last input and the first result at once: one device block, uploaded with the inputs and downloaded with the results.  Scratch may
// also lie between or behind results (layouts older than the phases); an input behind scratch or results clears `ordered`.
// The device offset of a block is Carver's; the pinned arena holds [inputs | mirror of the result span], so a result block at device
// offset off is read at inBytes + (off - oRes).  Both sizes are exact: nothing is placed behind them.
struct Staging {
    Carver c;
    size_t inBytes = 0, oRes = 0, resBytes = 0;
    bool hasRes = false, ordered = true;   // ordered: every input was taken before any scratch or result (reserve refuses otherwise)
    uint8_t *hp = nullptr, *dp = nullptr;

    template <class T> Block<T> in(size_t n) { ordered = ordered && !hasRes && c.off == inBytes; const Block<T> b = scratch<T>(n); inBytes = c.off; return b; }
    template <class T> Block<T> scratch(size_t n) { return Block<T>{c.take(n * sizeof(T)), n}; }
    template <class T> Block<T> out(size_t n) { if (!hasRes) { oRes = c.off; hasRes = true; } const Block<T> b = scratch<T>(n); resBytes = c.off - oRes; return b; }
    template <class T> Block<T> inout(size_t n) { ordered = ordered && !hasRes && c.off == inBytes; const Block<T> b = out<T>(n); inBytes = c.off; return b; }

    size_t device_bytes() const { return c.off; }
    size_t host_bytes() const { return inBytes + resBytes; }
    void bind(uint8_t* host, uint8_t* dev) { hp = host; dp = dev; }

    template <class T> T* host(Block<T> b) const { return reinterpret_cast<T*>(hp + b.off); }   // an input block, before the upload
    template <class T> T* dev(Block<T> b) const { return reinterpret_cast<T*>(dp + b.off); }
    template <class T> const T* res(Block<T> b) const { return reinterpret_cast<const T*>(hp + mirror(b.off)); }   // after the download
    size_t mirror(size_t off) const { return inBytes + (off - oRes); }

    // the copies into an input block and out of a result block; a null pointer or a zero count is a no-op
    template <class T> void put(Block<T> b, const void* src) const { put(b, src, b.n); }
    template <class T> void put(Block<T> b, const void* src, size_t count) const { if (src && count) memcpy(host(b), src, count * sizeof(T)); }
    template <class T> void get(Block<T> b, void* dst) const { get(b, dst, b.n); }
    template <class T> void get(Block<T> b, void* dst, size_t count) const { if (dst && count) memcpy(dst, res(b), count * sizeof(T)); }
};

}  // namespace orbfe
