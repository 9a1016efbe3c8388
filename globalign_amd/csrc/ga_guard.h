// ga_guard.h -- guard bands around the host engine's buffers: the layout arithmetic, the scan of a
// guard image and the report record.  No HIP here: ga_host.cpp allocates, fills and copies; ga_host_selftest.cpp
// drives this file alone on the CPU.
//
// A guarded allocation of a buffer whose kernels see `cap` payload bytes is
//
//     [ front guard: G ][ payload: cap ][ G more bytes ]
//
// with the payload pointer at raw + G.  G is a multiple of 256, so the payload keeps the allocator's 256-byte
// alignment.  The rear guard is the G bytes that begin where the most recent request ends -- raw + G + size, not
// raw + G + cap -- so it moves when a smaller problem reuses the buffer, and it always fits: size <= cap.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace gaguard {

constexpr size_t kAlign = 256;            // of the payload pointer, as an unguarded hipMalloc gives it
constexpr size_t kMaxGuard = 1u << 20;    // GA_GUARD_BYTES at most
constexpr unsigned kDefaultFill = 0xA5u;  // GA_GUARD_FILL

// GA_GUARD_BYTES as a context accepts it: 0 (off), or a multiple of 256 up to 1 MiB
inline bool valid_guard_bytes(long long g) { return g >= 0 && g <= (long long)kMaxGuard && g % (long long)kAlign == 0; }
inline bool valid_fill(long long f) { return f >= 0 && f <= 255; }

// raw allocation of a buffer of `cap` payload bytes
inline size_t alloc_bytes(size_t cap, size_t G) { return G + cap + G; }
inline size_t payload_off(size_t G) { return G; }
// raw offset of the rear guard's first byte for a request of `size` bytes (size <= cap)
inline size_t rear_off(size_t size, size_t G) { return G + size; }

// What re-laying the rear guard for a request of new_size bytes (after one of old_size) fills with the pattern, as
// payload offsets [lo, hi): what is left of the old guard and the new guard.  It never reaches below
// min(old, new), so the bytes both requests cover keep their contents.
struct Range {
    size_t lo, hi;
};
inline Range relay_range(size_t old_size, size_t new_size, size_t G) {
    return Range{std::min(old_size, new_size), std::max(old_size, new_size) + G};
}

enum Side { kFront = 0, kRear = 1 };

// A guard image's bytes that no longer hold the pattern: the first and the last one's index, and how many.
struct Scan {
    long long first = -1, last = -1;
    size_t changed = 0;
};
inline Scan scan(const uint8_t* img, size_t G, uint8_t fill) {
    Scan s;
    for (size_t k = 0; k < G; k++)
        if (img[k] != fill) {
            if (s.first < 0) s.first = (long long)k;
            s.last = (long long)k;
            s.changed++;
        }
    return s;
}

// One violated guard.  offset: the first changed byte relative to the payload's first byte -- negative in the front
// guard (-G .. -1), size .. size + G - 1 in the rear guard.
struct Violation {
    std::string name;
    int side = kFront;
    long long offset = 0;
    long long last = 0;  // the last changed byte, as offset
    size_t changed = 0;
    size_t payload = 0;  // the payload size at that moment (the last request)
};
inline long long rel_offset(int side, long long idx, size_t size, size_t G) {
    return side == kFront ? idx - (long long)G : (long long)size + idx;
}
inline bool make_violation(const std::string& name, int side, const Scan& s, size_t size, size_t G, Violation& v) {
    if (s.changed == 0) return false;
    v.name = name;
    v.side = side;
    v.offset = rel_offset(side, s.first, size, G);
    v.last = rel_offset(side, s.last, size, G);
    v.changed = s.changed;
    v.payload = size;
    return true;
}
// "colck rear +520 n=496 last=+1015 payload=33280"
inline std::string describe(const Violation& v) {
    auto sgn = [](long long x) { return (x < 0 ? "" : "+") + std::to_string(x); };
    return v.name + (v.side == kFront ? " front " : " rear ") + sgn(v.offset) + " n=" + std::to_string(v.changed) +
           " last=" + sgn(v.last) + " payload=" + std::to_string(v.payload);
}
inline std::string describe(const std::vector<Violation>& vs) {
    std::string s;
    for (const Violation& v : vs) s += (s.empty() ? "" : "; ") + describe(v);
    return s;
}

}  // namespace gaguard
