// lsr_host.h -- what every unit's host side shares: the error path (lsr::fail behind lsr_last_error,
// the check after a launch), workspace carving (one walk of a layout gives the *_bytes query and the
// pointers) and the gate on a public header's version.  Everything but fail is hidden from the
// library's exported symbols.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>

#include "../../include/lsr.h"

namespace lsr {

// sets the calling thread's lsr_last_error and returns code (lsr_api.hip)
int fail(int code, const std::string& msg);

#pragma GCC visibility push(hidden)

// after a kernel launch: LSR_OK, or LSR_EHIP and "<what>: <the HIP error>" (what: a literal or a
// std::string; the message is built only on failure)
template <typename S>
inline int launched(const S& what, hipError_t e = hipGetLastError()) {
    return e == hipSuccess ? LSR_OK : fail(LSR_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Bump allocator over a caller-owned workspace, every piece 256-byte aligned.  Over a null base it
// hands out null pointers and the same offsets: the same walk of a layout is its size query.
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* b = nullptr) : base(static_cast<char*>(b)) {}
    // the byte offset of the next piece
    size_t skip(size_t bytes) {
        const size_t at = off;
        off += align256(bytes);
        return at;
    }
    template <typename T>
    T* take(size_t n) {
        const size_t at = skip(n * sizeof(T));
        return base ? reinterpret_cast<T*>(base + at) : nullptr;
    }
    size_t total() const { return off; }
};

// The version of one public header that the caller declared it was built against (the header's
// *_require_api); the entry points that read the header's structs check it first.
struct ApiGate {
    const char *stem, *macro;    // "lsr_query" of lsr_query.h and lsr_query_require_api, "LSR_QUERY_API_VERSION"
    int32_t version;
    std::string built_against;   // how check() names what the caller must be built against
    std::atomic<int32_t> caller{0};
    int require(int32_t caller_version) {
        if (caller_version != version)
            return fail(LSR_EINVAL, std::string(stem) + ".h version mismatch: caller " + std::to_string(caller_version) +
                                        ", library " + std::to_string(version));
        caller.store(caller_version);
        return LSR_OK;
    }
    // what: the entry point's name, where its messages begin with it
    int check(const char* what = nullptr) const {
        if (caller.load() == version) return LSR_OK;
        return fail(LSR_EINVAL, (what ? std::string(what) + ": " : std::string()) + "call " + stem + "_require_api(" +
                                    macro + ") first: the caller must be built against " + built_against);
    }
};

#pragma GCC visibility pop

}  // namespace lsr
