// Test program (tests/test_sort_paths_gpu.py) for every path of the device scan and radix sort
// (4dlangsplat_amd/csrc/sort.hip) on exact integer data: each case is compared word for word with
// a host reference of the same operation (a running uint32_t sum; std::stable_sort of the kept ids
// by the key window; first / last + 1 position of every key below nranges; rect[value] and its
// rect_count).  Every case runs with the workspace filled with 0xA5 bytes, every output buffer
// prefilled with a sentinel plus 16 guard words, and checks that what the contract leaves unwritten
// ([kept, n) of the final buffers, out past n, the guards) is unchanged.
// Usage: t_sort_paths <scan|scan_batch|host_plan|ranges|depth_plan|batch>   one group on the device
//        t_sort_paths --selftest    no device call: every checker must accept a correct simulated
//                                   output and reject each of a list of single corruptions
// Exit 0: all cases ok, 1: a mismatch, 2: a HIP error (nothing further is run).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <numeric>
#include <random>
#include <string>
#include <utility>
#include <vector>
#include "../../4dlangsplat_amd/csrc/sort.hip"

namespace {

constexpr uint32_t SENT = 0x5E471E57u;     // prefill of outputs and guards
constexpr uint32_t POISON = 0xA5A5A5A5u;   // prefill of workspaces
constexpr size_t GUARD = 16;               // guard words past every buffer's end

#define CK(expr)                                                                                   \
    do {                                                                                           \
        const hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                                    \
            printf("HIP error: %s (%s) at line %d\n", hipGetErrorString(e_), #expr, __LINE__);     \
            fflush(stdout);                                                                        \
            std::_Exit(2);                                                                         \
        }                                                                                          \
    } while (0)

bool g_quiet = false;   // the self-test's corruption runs print no mismatch lines
int g_cases = 0, g_failed = 0;

struct Report {
    size_t bad = 0;
    void miss(const char* what, size_t i, uint32_t got, uint32_t want) {
        if (bad < 3 && !g_quiet) printf("  %s[%zu] got 0x%08x want 0x%08x\n", what, i, got, want);
        ++bad;
    }
};

bool verdict(const std::string& name, size_t n, const Report& r) {
    printf("%s n=%zu : %s\n", name.c_str(), n, r.bad ? "FAIL" : "ok");
    ++g_cases;
    if (r.bad) ++g_failed;
    return r.bad == 0;
}

// A buffer: its image before the call (pre) and after it (post), both [0, words + GUARD); on the
// device it starts `off` words past a 256-byte aligned allocation.
struct Buf {
    const char* name = "";
    size_t words = 0, off = 0;
    std::vector<uint32_t> pre, post;
    uint32_t* base = nullptr;
    uint32_t* d() const { return base + off; }
};

Buf make_buf(const char* name, size_t words, uint32_t fill, size_t off = 0) {
    Buf b;
    b.name = name;
    b.words = words;
    b.off = off;
    b.pre.assign(words + GUARD, fill);
    std::fill(b.pre.begin() + (ptrdiff_t)words, b.pre.end(), SENT);
    return b;
}
void upload(Buf& b) {
    CK(hipMalloc((void**)&b.base, (b.off + b.pre.size()) * 4));
    CK(hipMemcpy(b.d(), b.pre.data(), b.pre.size() * 4, hipMemcpyHostToDevice));
}
void download(Buf& b) {
    b.post.resize(b.pre.size());
    CK(hipMemcpy(b.post.data(), b.d(), b.post.size() * 4, hipMemcpyDeviceToHost));
}
void release(Buf& b) {
    if (b.base) CK(hipFree(b.base));
    b.base = nullptr;
}

// post == pre on [from, to)
void check_same(Report& r, const Buf& b, size_t from, size_t to) {
    for (size_t i = from; i < to; ++i)
        if (b.post[i] != b.pre[i]) r.miss(b.name, i, b.post[i], b.pre[i]);
}
void check_guard(Report& r, const Buf& b) { check_same(r, b, b.words, b.words + GUARD); }

// ---- scan ---------------------------------------------------------------------------------------
enum ScanData { ONES = 0, SMALL = 1, FULL = 2 };
const char* const kScanData[] = {"ones", "0..15", "u32"};

std::vector<uint32_t> scan_input(size_t n, int data, uint32_t seed) {
    std::mt19937 rng(seed);
    std::vector<uint32_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = data == ONES ? 1u : data == SMALL ? (uint32_t)(rng() & 15u) : (uint32_t)rng();
    return v;
}

// out[i] = in[0] + ... + in[i - 1] mod 2^32 for i < n, nothing written past n; total (if given)
void check_scan(Report& r, const std::vector<uint32_t>& in, const Buf& out, const Buf* total) {
    uint32_t run = 0;
    for (size_t i = 0; i < in.size(); ++i) {
        if (out.post[i] != run) r.miss("out", i, out.post[i], run);
        run += in[i];
    }
    check_guard(r, out);
    if (total) {
        if (total->post[0] != run) r.miss("total", 0, total->post[0], run);
        check_guard(r, *total);
    }
}

// a correct output made another way (each prefix summed in 64 bits, then truncated)
void simulate_scan(const std::vector<uint32_t>& in, Buf& out, Buf* total) {
    out.post = out.pre;
    uint64_t s = 0;
    for (size_t i = 0; i < in.size(); ++i) { out.post[i] = (uint32_t)(s & 0xFFFFFFFFull); s += in[i]; }
    if (total) { total->post = total->pre; total->post[0] = (uint32_t)(s & 0xFFFFFFFFull); }
}

struct ScanBufs {
    std::vector<uint32_t> in_host;
    Buf in, out, total, temp;
};
ScanBufs scan_bufs(size_t n, int data, uint32_t seed, size_t in_off = 0, size_t out_off = 0) {
    ScanBufs s;
    s.in_host = scan_input(n, data, seed);
    s.in = make_buf("in", n, 0u, in_off);
    std::copy(s.in_host.begin(), s.in_host.end(), s.in.pre.begin());
    s.out = make_buf("out", n, SENT, out_off);
    s.total = make_buf("total", 1, SENT);
    s.temp = make_buf("temp", lsr::scan_temp_bytes(n) / 4, POISON);   // exactly the workspace, then guards
    return s;
}
void upload(ScanBufs& s) { upload(s.in); upload(s.out); upload(s.total); upload(s.temp); }
void download(ScanBufs& s) { download(s.in); download(s.out); download(s.total); download(s.temp); }
void release(ScanBufs& s) { release(s.in); release(s.out); release(s.total); release(s.temp); }
void check_scan_bufs(Report& r, const ScanBufs& s, bool with_total) {
    check_scan(r, s.in_host, s.out, with_total ? &s.total : nullptr);
    if (!with_total) check_same(r, s.total, 0, 1 + GUARD);
    check_same(r, s.in, 0, s.in.words + GUARD);
    check_guard(r, s.temp);
}

void run_scan_case(size_t n, int data, bool with_total, size_t in_off, size_t out_off) {
    ScanBufs s = scan_bufs(n, data, 77u + (uint32_t)n, in_off, out_off);
    upload(s);
    lsr::exclusive_scan_u32(s.in.d(), s.out.d(), n, with_total ? s.total.d() : nullptr, s.temp.d(), 0);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    download(s);
    Report r;
    check_scan_bufs(r, s, with_total);
    char name[96];
    snprintf(name, sizeof name, "scan %s total=%d in+%zu out+%zu", kScanData[data], (int)with_total, in_off, out_off);
    verdict(name, n, r);
    release(s);
}

void group_scan() {
    const size_t sizes[] = {0, 1, 7, 8, 9, 2047, 2048, 2049, 4095, 4096, 4097, 526341, 8388608, 8388609};
    for (size_t n : sizes)
        for (int data = 0; data < 3; ++data)
            for (int t = 1; t >= 0; --t) run_scan_case(n, data, t != 0, 0, 0);
    // scalar branches of the loads and of the store: in 1 word, out 3 words past a 256-byte boundary
    for (size_t n : {(size_t)2049, (size_t)4097})
        for (int data = 0; data < 3; ++data) {
            run_scan_case(n, data, true, 1, 0);
            run_scan_case(n, data, true, 0, 3);
            run_scan_case(n, data, true, 1, 3);
        }
}

bool scan_batch_once(const std::vector<size_t>& ns, const char* tag) {
    const int nseg = (int)ns.size();
    std::vector<ScanBufs> s(nseg);
    uint32_t* host_words = nullptr;   // mapped pinned: one word per segment, then guards
    CK(hipHostMalloc((void**)&host_words, (nseg + GUARD) * 4, hipHostMallocMapped));
    for (size_t i = 0; i < nseg + GUARD; ++i) host_words[i] = SENT;
    void* mapped = nullptr;
    CK(hipHostGetDevicePointer(&mapped, host_words, 0));
    lsr::ScanSeg segs[lsr::LSR_MAX_VIEWS];
    uint32_t want_mask = 0;
    for (int i = 0; i < nseg; ++i) {
        s[i] = scan_bufs(ns[i], (int)(ns[i] % 3), 1000u + (uint32_t)ns[i]);
        upload(s[i]);
        segs[i] = lsr::ScanSeg{s[i].in.d(), s[i].out.d(), s[i].total.d(), s[i].temp.d(), ns[i],
                               static_cast<uint32_t*>(mapped) + i};
        if (ns[i] > 2048 && ns[i] <= 8388608) want_mask |= 1u << i;
    }
    const uint32_t mask = lsr::exclusive_scan_batch(segs, nseg, 0);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(0));
    CK(hipDeviceSynchronize());
    bool ok = true;
    {
        Report r;
        if (mask != want_mask) r.miss("mask", 0, mask, want_mask);
        for (size_t i = nseg; i < nseg + GUARD; ++i)
            if (host_words[i] != SENT) r.miss("host_total guard", i, host_words[i], SENT);
        ok &= verdict(std::string("scan_batch ") + tag + " mask", (size_t)nseg, r);
    }
    for (int i = 0; i < nseg; ++i) {
        download(s[i]);
        Report r;
        check_scan_bufs(r, s[i], true);
        uint32_t sum = 0;
        for (uint32_t x : s[i].in_host) sum += x;
        const uint32_t want = (want_mask >> i & 1u) ? sum : SENT;   // unwritten words keep the sentinel
        if (host_words[i] != want) r.miss("host_total", (size_t)i, host_words[i], want);
        char name[64];
        snprintf(name, sizeof name, "scan_batch %s seg %d %s", tag, i, kScanData[ns[i] % 3]);
        ok &= verdict(name, ns[i], r);
        release(s[i]);
    }
    CK(hipHostFree(host_words));
    return ok;
}

void group_scan_batch() {
    std::vector<size_t> ns = {0, 1, 2048, 2049, 5000, 100000, 526341, 8388609};
    scan_batch_once(ns, "fwd");
    std::reverse(ns.begin(), ns.end());   // segment index != index among the two-kernel segments
    scan_batch_once(ns, "rev");
}

// ---- sort ---------------------------------------------------------------------------------------
struct SortCase {
    std::string name;
    size_t n = 0;
    int begin = 0, end = 32;
    std::vector<uint32_t> keys, vals;
    bool use_kept = false;   // kept word given: keys equal to 0xFFFFFFFF are dropped
    bool planned = false;    // vals_c and gather given: the device-planned depth sort
    uint32_t nranges = 0;    // > 0: ranges given
    std::vector<uint32_t> rect;   // planned: rect[id] as two words
    int want_three = -1;     // planned: the plan named by the case list (-1: only the plan rule is checked)
    uint32_t want_kbase = 0;
};

struct SortBufs {
    Buf ka, va, kb, vb, vc, kept, ranges, rect, rs, cnt, temp;
    std::vector<Buf*> all() { return {&ka, &va, &kb, &vb, &vc, &kept, &ranges, &rect, &rs, &cnt, &temp}; }
    std::vector<const Buf*> all() const { return {&ka, &va, &kb, &vb, &vc, &kept, &ranges, &rect, &rs, &cnt, &temp}; }
};

SortBufs sort_bufs(const SortCase& c) {
    SortBufs b;
    const size_t n = c.n;
    b.ka = make_buf("keys_a", n, 0u);
    std::copy(c.keys.begin(), c.keys.end(), b.ka.pre.begin());
    b.va = make_buf("vals_a", n, 0u);
    std::copy(c.vals.begin(), c.vals.end(), b.va.pre.begin());
    b.kb = make_buf("keys_b", n, SENT);
    b.vb = make_buf("vals_b", n, SENT);
    b.vc = make_buf("vals_c", c.planned ? n : 0, SENT);
    b.kept = make_buf("kept", 1, SENT);
    b.ranges = make_buf("ranges", 2 * (size_t)c.nranges, 0u);
    for (size_t k = 0; k < c.nranges; ++k) b.ranges.pre[2 * k] = 0xFFFFFFFFu;   // preset (0xFFFFFFFF, 0)
    b.rect = make_buf("rect", c.planned ? 2 * n : 0, 0u);
    std::copy(c.rect.begin(), c.rect.end(), b.rect.pre.begin());
    b.rs = make_buf("rect_sorted", c.planned ? 2 * n : 0, SENT);
    b.cnt = make_buf("counts", c.planned ? n : 0, SENT);
    b.temp = make_buf("temp", lsr::radix_temp_bytes(n) / 4, POISON);   // exactly the workspace, then guards
    return b;
}
void upload(SortBufs& b) { for (Buf* p : b.all()) upload(*p); }
void download(SortBufs& b) { for (Buf* p : b.all()) download(*p); }
void release(SortBufs& b) { for (Buf* p : b.all()) release(*p); }

uint32_t window(uint32_t key, int begin, int end) {
    const int w = end - begin;
    return w >= 32 ? key : (key >> begin) & ((1u << w) - 1u);
}

struct SortRef {
    std::vector<uint32_t> pos;   // input positions of the kept pairs in sorted order
    int in_b = 0;
    uint32_t three = 0, kbase = 0;
};
SortRef sort_ref(const SortCase& c) {
    SortRef f;
    f.pos.reserve(c.n);
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (size_t i = 0; i < c.n; ++i) {
        if (c.use_kept && c.keys[i] == 0xFFFFFFFFu) continue;
        f.pos.push_back((uint32_t)i);
        lo = std::min(lo, c.keys[i]);
        hi = std::max(hi, c.keys[i]);
    }
    const int b = c.begin, e = c.end;
    std::stable_sort(f.pos.begin(), f.pos.end(),
                     [&](uint32_t x, uint32_t y) { return window(c.keys[x], b, e) < window(c.keys[y], b, e); });
    if (c.planned) {
        // the plan rule: kbase = lo & ~0xFF, three passes (8 + 9 + 9 bits) when hi - kbase < 2^26
        const uint32_t kb = lo & ~0xFFu;
        f.three = (!f.pos.empty() && hi - kb < (1u << 26)) ? 1u : 0u;
        f.kbase = f.three ? kb : 0u;
        f.in_b = 0;
    } else {
        f.in_b = ((e - b + 7) / 8) & 1;   // one buffer swap per pass
    }
    return f;
}

// ret: what the sort returned (0: result in a, 1: in b).  An empty segment (of a batch) must leave
// every buffer as it was.
void check_sort(Report& r, const SortCase& c, const SortBufs& b, int ret) {
    for (const Buf* p : b.all()) check_guard(r, *p);
    check_same(r, b.rect, 0, b.rect.words);
    if (c.n == 0) {
        for (const Buf* p : b.all()) check_same(r, *p, 0, p->words);
        return;
    }
    const SortRef f = sort_ref(c);
    const size_t n = c.n, nk = f.pos.size();
    if (ret != f.in_b) r.miss("returned buffer", 0, (uint32_t)ret, (uint32_t)f.in_b);
    if (c.use_kept) {
        if (b.kept.post[0] != (uint32_t)nk) r.miss("kept", 0, b.kept.post[0], (uint32_t)nk);
    } else {
        check_same(r, b.kept, 0, 1);
    }
    const Buf& fk = f.in_b ? b.kb : b.ka;
    const Buf& fv = f.in_b ? b.vb : b.va;
    for (size_t i = 0; i < nk; ++i) {
        const uint32_t p = f.pos[i];
        if (fv.post[i] != c.vals[p]) r.miss(fv.name, i, fv.post[i], c.vals[p]);
        if (!c.planned && fk.post[i] != c.keys[p]) r.miss(fk.name, i, fk.post[i], c.keys[p]);   // planned: keys unspecified
    }
    check_same(r, fv, nk, n);
    if (!c.planned) check_same(r, fk, nk, n);
    if (c.nranges) {
        std::vector<uint32_t> want(b.ranges.pre.begin(), b.ranges.pre.begin() + 2 * (ptrdiff_t)c.nranges);
        for (size_t i = 0; i < nk; ++i) {
            const uint32_t k = c.keys[f.pos[i]];
            if (k >= c.nranges) continue;
            want[2 * k] = std::min(want[2 * k], (uint32_t)i);
            want[2 * k + 1] = std::max(want[2 * k + 1], (uint32_t)i + 1u);
        }
        for (size_t i = 0; i < want.size(); ++i)
            if (b.ranges.post[i] != want[i]) r.miss(i & 1 ? "ranges.end" : "ranges.start", i / 2, b.ranges.post[i], want[i]);
    }
    if (c.planned) {
        for (size_t i = 0; i < nk; ++i) {
            const uint32_t id = c.vals[f.pos[i]];
            const uint2 rc = make_uint2(c.rect[2 * (size_t)id], c.rect[2 * (size_t)id + 1]);
            if (b.rs.post[2 * i] != rc.x) r.miss("rect_sorted.x", i, b.rs.post[2 * i], rc.x);
            if (b.rs.post[2 * i + 1] != rc.y) r.miss("rect_sorted.y", i, b.rs.post[2 * i + 1], rc.y);
            const uint32_t cnt = lsr::rect_count(rc);
            if (b.cnt.post[i] != cnt) r.miss("counts", i, b.cnt.post[i], cnt);
        }
        check_same(r, b.rs, 2 * nk, 2 * n);     // the culled ranks keep what they had
        check_same(r, b.cnt, nk, n);
        const size_t pw = lsr::RTS_PLAN_OFF / 4;
        if (b.temp.post[pw] != f.kbase) r.miss("plan kbase", 0, b.temp.post[pw], f.kbase);
        if (b.temp.post[pw + 1] != f.three) r.miss("plan three-pass flag", 0, b.temp.post[pw + 1], f.three);
        if (c.want_three >= 0) {
            if (b.temp.post[pw] != c.want_kbase) r.miss("named plan kbase", 0, b.temp.post[pw], c.want_kbase);
            if (b.temp.post[pw + 1] != (uint32_t)c.want_three)
                r.miss("named plan three-pass flag", 0, b.temp.post[pw + 1], (uint32_t)c.want_three);
        }
    }
}

// A correct output made another way: an unstable sort of (window, input position) pairs, ranges by
// a search per key; the device's plan words by the rule.  Intermediate buffers keep their prefill.
void simulate_sort(const SortCase& c, SortBufs& b, int* ret) {
    for (Buf* p : b.all()) p->post = p->pre;
    std::vector<std::pair<uint32_t, uint32_t>> pr;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (size_t i = 0; i < c.n; ++i)
        if (!(c.use_kept && c.keys[i] == 0xFFFFFFFFu)) {
            pr.emplace_back(window(c.keys[i], c.begin, c.end), (uint32_t)i);
            lo = std::min(lo, c.keys[i]);
            hi = std::max(hi, c.keys[i]);
        }
    std::sort(pr.begin(), pr.end());
    int passes = 0;
    for (int s = c.begin; s < c.end; s += 8) ++passes;
    *ret = c.planned ? 0 : passes % 2;
    Buf& fk = *ret ? b.kb : b.ka;
    Buf& fv = *ret ? b.vb : b.va;
    if (c.use_kept) b.kept.post[0] = (uint32_t)pr.size();
    for (size_t i = 0; i < pr.size(); ++i) {
        const uint32_t p = pr[i].second;
        fv.post[i] = c.vals[p];
        if (!c.planned) fk.post[i] = c.keys[p];
        if (c.planned) {
            b.rs.post[2 * i] = c.rect[2 * (size_t)c.vals[p]];
            b.rs.post[2 * i + 1] = c.rect[2 * (size_t)c.vals[p] + 1];
            b.cnt.post[i] = lsr::rect_count(make_uint2(b.rs.post[2 * i], b.rs.post[2 * i + 1]));
        }
    }
    for (uint32_t k = 0; k < c.nranges; ++k) {
        size_t first = pr.size(), last = 0;
        for (size_t i = 0; i < pr.size(); ++i)
            if (c.keys[pr[i].second] == k) { first = std::min(first, i); last = i + 1; }
        if (last) { b.ranges.post[2 * k] = (uint32_t)first; b.ranges.post[2 * k + 1] = (uint32_t)last; }
    }
    if (c.planned) {
        const bool three = !pr.empty() && hi - (lo & ~0xFFu) < 0x4000000u;
        b.temp.post[lsr::RTS_PLAN_OFF / 4] = three ? (lo & ~0xFFu) : 0u;
        b.temp.post[lsr::RTS_PLAN_OFF / 4 + 1] = three ? 1u : 0u;
    }
}

lsr::SortSeg seg_of(const SortCase& c, SortBufs& b) {
    lsr::SortSeg sg{b.ka.d(), b.va.d(), b.kb.d(), b.vb.d(), b.temp.d(), c.use_kept ? b.kept.d() : nullptr,
                    lsr::SortGather{nullptr, nullptr, nullptr}, c.n};
    if (c.planned) {
        sg.gather = lsr::SortGather{reinterpret_cast<const uint2*>(b.rect.d()), b.cnt.d(), reinterpret_cast<uint2*>(b.rs.d())};
        sg.vals_c = b.vc.d();
    }
    if (c.nranges) {
        sg.ranges = reinterpret_cast<uint2*>(b.ranges.d());
        sg.nranges = c.nranges;
    }
    return sg;
}

// radix_sort_pairs has no ranges argument: cases with ranges go through a batch of one
bool run_sort_case(const SortCase& c) {
    SortBufs b = sort_bufs(c);
    upload(b);
    int ret;
    if (c.nranges) {
        const lsr::SortSeg sg = seg_of(c, b);
        ret = lsr::radix_sort_batch(&sg, 1, c.begin, c.end, 0);
    } else {
        const lsr::SortGather g{reinterpret_cast<const uint2*>(b.rect.d()), b.cnt.d(), reinterpret_cast<uint2*>(b.rs.d())};
        ret = lsr::radix_sort_pairs(b.ka.d(), b.va.d(), b.kb.d(), b.vb.d(), c.n, c.begin, c.end, b.temp.d(), 0,
                                    c.use_kept ? b.kept.d() : nullptr, c.planned ? &g : nullptr,
                                    c.planned ? b.vc.d() : nullptr)
                  ? 1 : 0;
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    download(b);
    Report r;
    check_sort(r, c, b, ret);
    const bool ok = verdict(c.name, c.n, r);
    release(b);
    return ok;
}

// values: a fixed shuffle of the ids, so that a value differs from its position
std::vector<uint32_t> shuffled_ids(size_t n, uint32_t seed) {
    std::vector<uint32_t> v(n);
    std::iota(v.begin(), v.end(), 0u);
    std::mt19937 rng(seed);
    for (size_t i = n; i > 1; --i) std::swap(v[i - 1], v[rng() % i]);
    return v;
}

enum Pattern { P_RANDOM, P_EQUAL, P_ASC, P_DESC, P_ALT };
const char* const kPattern[] = {"random", "equal", "ascending", "descending", "alternating"};
enum Share { S_NONE = 0, S_TENTH = 1, S_ALL_BUT_ONE = 2, S_ALL = 3 };
const char* const kShare[] = {"0", "10%", "all-but-one", "all"};

// drop keys (set them to 0xFFFFFFFF); `protect` lists positions a 10 % share must keep, and
// protect[0] is the one position "all but one" keeps
void drop_keys(std::vector<uint32_t>& keys, int share, std::mt19937& rng, const std::vector<size_t>& protect) {
    const size_t n = keys.size();
    for (size_t i = 0; i < n; ++i) {
        const bool prot = std::find(protect.begin(), protect.end(), i) != protect.end();
        bool drop = false;
        if (share == S_TENTH) drop = rng() % 10 == 0 && !prot;
        if (share == S_ALL_BUT_ONE) drop = i != (protect.empty() ? n / 2 : protect[0]);
        if (share == S_ALL) drop = true;
        if (drop) keys[i] = 0xFFFFFFFFu;
    }
}

// host-planned keys: `pattern` inside the window [begin, end), random bits outside it
SortCase host_case(const std::string& name, size_t n, int begin, int end, int pattern, bool use_kept, int share,
                   uint32_t seed) {
    SortCase c;
    c.name = name;
    c.n = n;
    c.begin = begin;
    c.end = end;
    c.use_kept = use_kept;
    c.vals = shuffled_ids(n, seed ^ 0x9E3779B9u);
    c.keys.resize(n);
    std::mt19937 rng(seed);
    const int w = end - begin;
    const uint32_t wmask = w >= 32 ? 0xFFFFFFFFu : (1u << w) - 1u;
    const uint32_t e0 = (uint32_t)rng() & wmask, a0 = (uint32_t)rng() & wmask, a1 = ~a0 & wmask;
    for (size_t i = 0; i < n; ++i) {
        uint32_t d = 0;
        if (pattern == P_RANDOM) d = (uint32_t)rng() & wmask;
        if (pattern == P_EQUAL) d = e0;
        if (pattern == P_ASC) d = (uint32_t)((uint64_t)i * ((uint64_t)wmask + 1) / n);
        if (pattern == P_DESC) d = (uint32_t)((uint64_t)(n - 1 - i) * ((uint64_t)wmask + 1) / n);
        if (pattern == P_ALT) d = ((i & 1) ? a1 : a0) & wmask;
        const uint32_t outside = w >= 32 ? 0u : (uint32_t)rng() & ~(wmask << begin);
        c.keys[i] = (d << begin) | outside;
    }
    if (use_kept) drop_keys(c.keys, share, rng, {});
    return c;
}

std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char* f, ...) {
    char buf[160];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

void group_host_plan() {
    const size_t sizes[] = {1, 63, 64, 65, 255, 256, 2047, 2048, 2049, 4097, 40000};
    for (size_t n : sizes)
        for (int end : {13, 32})
            run_sort_case(host_case(fmt("host_plan sizes [0,%d)", end), n, 0, end, P_RANDOM, false, 0, 11u + (uint32_t)n));
    const int windows[][2] = {{0, 1}, {0, 5}, {0, 8}, {0, 9}, {0, 16}, {0, 17}, {0, 30}, {3, 16}, {19, 32}};
    for (const auto& w : windows)
        for (size_t n : {(size_t)4097, (size_t)40000})
            run_sort_case(host_case(fmt("host_plan window [%d,%d)", w[0], w[1]), n, w[0], w[1], P_RANDOM, false, 0,
                                    23u + (uint32_t)n + 64u * (uint32_t)w[1]));
    for (int p = P_RANDOM; p <= P_ALT; ++p)
        for (size_t n : {(size_t)4097, (size_t)40000})
            run_sort_case(host_case(fmt("host_plan pattern %s [0,13)", kPattern[p]), n, 0, 13, p, false, 0, 37u + (uint32_t)n));
    for (size_t n : {(size_t)4097, (size_t)40000})
        for (int share = S_NONE; share <= S_ALL; ++share)
            for (int end : {8, 13})   // one pass (result in b) and two passes (result in a)
                run_sort_case(host_case(fmt("host_plan kept dropped=%s [0,%d)", kShare[share], end), n, 0, end, P_RANDOM, true,
                                        share, 41u + (uint32_t)n + (uint32_t)share));
    // the first size with 12 keys per thread
    run_sort_case(host_case("host_plan 12-per-thread [0,13)", 4194305, 0, 13, P_RANDOM, false, 0, 53u));
}

// tile-like keys in [0, kmax) (nothing outside the window), one id never used
SortCase ranges_case(const std::string& name, size_t n, int end, uint32_t nranges, uint32_t kmax, uint32_t unused,
                     bool dropped, uint32_t seed) {
    SortCase c;
    c.name = name;
    c.n = n;
    c.begin = 0;
    c.end = end;
    c.use_kept = dropped;
    c.nranges = nranges;
    c.vals = shuffled_ids(n, seed ^ 0x9E3779B9u);
    c.keys.resize(n);
    std::mt19937 rng(seed);
    for (size_t i = 0; i < n; ++i) {
        uint32_t k = (uint32_t)(rng() % kmax);
        if (k == unused) k = (k + 1) % kmax;
        c.keys[i] = k;
    }
    if (dropped) drop_keys(c.keys, S_TENTH, rng, {});
    return c;
}

void group_ranges() {
    for (size_t n : {(size_t)300, (size_t)4097, (size_t)40000})
        for (int dropped = 0; dropped < 2; ++dropped) {
            const uint32_t seed = 61u + (uint32_t)n + (uint32_t)dropped;
            run_sort_case(ranges_case(fmt("ranges nranges=6 [0,3) dropped=%d", dropped), n, 3, 6, 8, 3, dropped != 0, seed));
            run_sort_case(ranges_case(fmt("ranges nranges=5440 [0,13) dropped=%d", dropped), n, 13, 5440, 5440, 1234,
                                      dropped != 0, seed + 1));
            run_sort_case(ranges_case(fmt("ranges nranges=5000 keys<8192 [0,13) dropped=%d", dropped), n, 13, 5000, 8192,
                                      77, dropped != 0, seed + 2));
        }
}

uint32_t float_bits(float z) {
    uint32_t b;
    std::memcpy(&b, &z, 4);
    return b;
}

// binning rectangles by id: culled (zero), at most 2 x 2 tiles with a random quadrant map, larger
std::vector<uint32_t> make_rects(size_t n, uint32_t seed) {
    std::mt19937 rng(seed);
    std::vector<uint32_t> r(2 * n);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t kind = rng() % 8;
        uint2 rc = make_uint2(0u, 0u);
        const uint32_t x0 = rng() % 300, y0 = rng() % 200;
        if (kind >= 1 && kind <= 4) rc = lsr::rect_pack(x0, y0, x0 + 1 + rng() % 2, y0 + 1 + rng() % 2, rng() & 0xFFFFu);
        if (kind >= 5) rc = lsr::rect_pack(x0, y0, x0 + 1 + rng() % 9, y0 + 3 + rng() % 7, 0u);
        r[2 * i] = rc.x;
        r[2 * i + 1] = rc.y;
    }
    return r;
}

enum KeySet { K_A, K_B, K_C, K_D, K_E_FF, K_E_00, K_F, K_G, K_H };
const char* const kKeySet[] = {"a", "b", "c", "d", "e-ff", "e-00", "f", "g", "h"};

// the depth sort's key sets (see the group's list); share: the culled share
SortCase depth_case(const std::string& group, size_t n, int set, int share, uint32_t seed) {
    SortCase c;
    c.name = fmt("%s set=%s culled=%s", group.c_str(), kKeySet[set], kShare[share]);
    c.n = n;
    c.use_kept = true;
    c.planned = true;
    c.vals = shuffled_ids(n, seed ^ 0x9E3779B9u);
    c.rect = make_rects(n, seed ^ 0x7F4A7C15u);
    c.keys.resize(n);
    std::mt19937 rng(seed);
    const size_t pmin = n / 3, pmax = n >= 2 ? (pmin + 1 + (2 * n / 5)) % n : 0;   // where the extremes sit
    uint32_t lo = 0, hi = 0;   // boundary sets: the smallest and the largest key
    if (set == K_C) { lo = 0x40000123u; hi = 0x40000100u + (1u << 26) - 1u; }
    if (set == K_D) { lo = 0x40000123u; hi = 0x40000100u + (1u << 26); }   // one past the three-pass plan's reach
    if (set == K_E_FF) { lo = 0x400001FFu; hi = 0x40000100u + (1u << 26) - 1u; }
    if (set == K_E_00) { lo = 0x40000200u; hi = 0x40000200u + (1u << 26) - 1u; }
    for (size_t i = 0; i < n; ++i) {
        const float z = 2.0f + 8.0f * (float)(rng() & 0xFFFFFF) / 16777216.0f;
        uint32_t k = 0;
        switch (set) {
            case K_A: k = float_bits(z); break;
            case K_B: k = float_bits(i % 7 == 6 ? z * 300.0f : z); break;
            case K_F: k = (uint32_t)(rng() % 0xFFFFFFFFu); break;
            case K_G: k = 0x40490FDBu; break;
            case K_H: k = float_bits(2.0f + 8.0f * (float)(rng() % 64) / 64.0f); break;
            default: k = lo + (uint32_t)(rng() % (hi - lo + 1u)); break;
        }
        c.keys[i] = k;
    }
    if (lo) {
        c.keys[pmax] = hi;
        c.keys[pmin] = lo;
    }
    drop_keys(c.keys, share, rng, {pmin, pmax});
    // the plans the case list names
    const bool some = share != S_ALL, both = share <= S_TENTH && n >= 2;
    if (!some) { c.want_three = 0; c.want_kbase = 0; }
    else if (set == K_C) { c.want_three = 1; c.want_kbase = 0x40000100u; }   // all-but-one keeps the smallest
    else if (set == K_D && both) { c.want_three = 0; c.want_kbase = 0; }
    else if (set == K_F && both && n >= 64) { c.want_three = 0; c.want_kbase = 0; }
    else if (set == K_A) {
        uint32_t kmin = 0xFFFFFFFFu;   // 0xFFFFFFFF itself is a culled key
        for (uint32_t k : c.keys) kmin = std::min(kmin, k);
        c.want_three = 1;
        c.want_kbase = kmin & ~0xFFu;
    }
    else if (set == K_G) { c.want_three = 1; c.want_kbase = 0x40490F00u; }
    return c;
}

void group_depth_plan() {
    const size_t sizes[] = {1, 64, 65, 3071, 3072, 3073, 9233, 50000};
    for (size_t n : sizes)
        for (int set : {K_A, K_B, K_F, K_H})
            for (int share = S_NONE; share <= S_ALL; ++share)
                run_sort_case(depth_case("depth_plan", n, set, share, 71u + (uint32_t)n + 16u * (uint32_t)set + (uint32_t)share));
    for (size_t n : {(size_t)9233, (size_t)50000})
        for (int set : {K_C, K_D, K_E_FF, K_E_00, K_G})
            for (int share = S_NONE; share <= S_ALL; ++share)
                run_sort_case(depth_case("depth_plan", n, set, share, 71u + (uint32_t)n + 16u * (uint32_t)set + (uint32_t)share));
    // 2049 count rows of 3072 keys: the scan's second chunk of rows, with 9-bit digits (three-pass plan)
    run_sort_case(depth_case("depth_plan 2049-rows", 6291457, K_A, S_TENTH, 83u));
}

// ---- batches ------------------------------------------------------------------------------------
bool run_batch(const char* tag, std::vector<SortCase>& cs, int begin, int end) {
    const int nseg = (int)cs.size();
    std::vector<SortBufs> bs(nseg);
    lsr::SortSeg segs[lsr::LSR_MAX_VIEWS];
    for (int i = 0; i < nseg; ++i) {
        bs[i] = sort_bufs(cs[i]);   // own buffers, and a workspace of exactly radix_temp_bytes(own n)
        upload(bs[i]);
        segs[i] = seg_of(cs[i], bs[i]);
    }
    const int ret = lsr::radix_sort_batch(segs, nseg, begin, end, 0);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    bool ok = true;
    for (int i = 0; i < nseg; ++i) {
        download(bs[i]);
        Report r;
        check_sort(r, cs[i], bs[i], ret);
        ok &= verdict(fmt("batch %s seg %d %s", tag, i, cs[i].name.c_str()), cs[i].n, r);
        release(bs[i]);
    }
    return ok;
}

// a call that must return -1 and leave every buffer and workspace as it was
bool run_refusal(const char* tag, std::vector<SortCase>& cs, int begin, int end,
                 const std::function<void(lsr::SortSeg*)>& edit) {
    const int nseg = (int)cs.size();
    std::vector<SortBufs> bs(nseg);
    lsr::SortSeg segs[lsr::LSR_MAX_VIEWS];
    for (int i = 0; i < nseg; ++i) {
        bs[i] = sort_bufs(cs[i]);
        upload(bs[i]);
        segs[i] = seg_of(cs[i], bs[i]);
    }
    edit(segs);
    const int ret = lsr::radix_sort_batch(segs, nseg, begin, end, 0);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    Report r;
    if (ret != -1) r.miss("return value", 0, (uint32_t)ret, (uint32_t)-1);
    for (int i = 0; i < nseg; ++i) {
        download(bs[i]);
        for (const Buf* p : bs[i].all()) check_same(r, *p, 0, p->words + GUARD);
        release(bs[i]);
    }
    return verdict(fmt("batch refusal %s", tag), cs[0].n, r);
}

void group_batch() {
    {   // host-planned with ranges and kept; the largest segment puts every one on 12 keys per thread
        const size_t ns[] = {0, 1, 2049, 3073, 40000, 4194305, 17, 4097};
        std::vector<SortCase> cs;
        for (size_t n : ns) cs.push_back(ranges_case("nranges=5440 [0,13) dropped=1", n, 13, 5440, 5440, 1234, true, 91u + (uint32_t)n));
        run_batch("host", cs, 0, 13);
    }
    {   // device-planned; key sets (a) and (b) alternate, so both plans run in one batch
        const size_t ns[] = {3073, 0, 1, 50000, 9233, 64, 3072, 12289};
        std::vector<SortCase> cs;
        for (int i = 0; i < 8; ++i) cs.push_back(depth_case("planned", ns[i], (i & 1) ? K_B : K_A, S_TENTH, 97u + (uint32_t)ns[i]));
        run_batch("planned", cs, 0, 32);
    }
    auto two_planned = [] {
        std::vector<SortCase> cs;
        cs.push_back(depth_case("planned", 3073, K_A, S_TENTH, 101u));
        cs.push_back(depth_case("planned", 9233, K_B, S_TENTH, 103u));
        return cs;
    };
    {
        std::vector<SortCase> cs = two_planned();
        run_refusal("planned + host-planned", cs, 0, 32, [](lsr::SortSeg* s) {
            s[1].vals_c = nullptr;
            s[1].gather = lsr::SortGather{nullptr, nullptr, nullptr};
        });
    }
    { std::vector<SortCase> cs = two_planned(); run_refusal("planned over [0,16)", cs, 0, 16, [](lsr::SortSeg*) {}); }
    { std::vector<SortCase> cs = two_planned(); run_refusal("planned without gather.rect", cs, 0, 32, [](lsr::SortSeg* s) { s[1].gather.rect = nullptr; }); }
    { std::vector<SortCase> cs = two_planned(); run_refusal("planned without gather.counts", cs, 0, 32, [](lsr::SortSeg* s) { s[0].gather.counts = nullptr; }); }
    { std::vector<SortCase> cs = two_planned(); run_refusal("planned without gather.rect_sorted", cs, 0, 32, [](lsr::SortSeg* s) { s[1].gather.rect_sorted = nullptr; }); }
    { std::vector<SortCase> cs = two_planned(); run_refusal("planned without gather", cs, 0, 32, [](lsr::SortSeg* s) { s[0].gather = lsr::SortGather{nullptr, nullptr, nullptr}; }); }
    { std::vector<SortCase> cs = two_planned(); run_refusal("planned without kept", cs, 0, 32, [](lsr::SortSeg* s) { s[1].kept = nullptr; }); }
}

// ---- self-test (no device call) -----------------------------------------------------------------
int g_self_bad = 0;
void expect(bool cond, const std::string& what) {
    printf("selftest %s : %s\n", what.c_str(), cond ? "ok" : "FAIL");
    if (!cond) ++g_self_bad;
}

// the checker accepts the simulated output, and rejects it after each corruption alone
using SortEdit = std::function<bool(const SortCase&, SortBufs&, const SortRef&)>;   // false: could not apply
void selftest_sort(const SortCase& c, const std::vector<std::pair<std::string, SortEdit>>& edits) {
    SortBufs b = sort_bufs(c);
    int ret = 0;
    simulate_sort(c, b, &ret);
    const SortRef f = sort_ref(c);
    {
        Report r;
        check_sort(r, c, b, ret);
        expect(r.bad == 0, c.name + ": correct output accepted");
    }
    {
        Report r;
        g_quiet = true;
        check_sort(r, c, b, ret ^ 1);
        g_quiet = false;
        expect(r.bad != 0, c.name + ": wrong returned buffer rejected");
    }
    for (const auto& e : edits) {
        SortBufs x = b;
        const bool applied = e.second(c, x, f);
        Report r;
        g_quiet = true;
        check_sort(r, c, x, ret);
        g_quiet = false;
        expect(applied && r.bad != 0, c.name + ": " + e.first + " rejected");
    }
}

int selftest() {
    // scan
    for (size_t n : {(size_t)0, (size_t)1, (size_t)5000}) {
        ScanBufs s = scan_bufs(n, FULL, 5u);
        for (Buf* p : {&s.in, &s.temp}) p->post = p->pre;
        simulate_scan(s.in_host, s.out, &s.total);
        Report r;
        check_scan_bufs(r, s, true);
        expect(r.bad == 0, fmt("scan n=%zu: correct output accepted", n));
        auto rejected = [&](const std::function<void(ScanBufs&)>& edit) {
            ScanBufs x = s;
            edit(x);
            Report q;
            g_quiet = true;
            check_scan_bufs(q, x, true);
            g_quiet = false;
            return q.bad != 0;
        };
        if (n > 1)
            expect(rejected([&](ScanBufs& x) { for (size_t i = n / 2; i < n; ++i) x.out.post[i] += 1u; }),
                   fmt("scan n=%zu: off by one from an index on rejected", n));
        if (n > 1)
            expect(rejected([&](ScanBufs& x) { x.out.post[n - 1] -= 1u; }), fmt("scan n=%zu: last value off by one rejected", n));
        expect(rejected([](ScanBufs& x) { x.total.post[0] += 1u; }), fmt("scan n=%zu: wrong total rejected", n));
        expect(rejected([&](ScanBufs& x) { x.out.post[n] = 0u; }), fmt("scan n=%zu: word past n written rejected", n));
        expect(rejected([&](ScanBufs& x) { x.out.post[n + GUARD - 1] = 0u; }), fmt("scan n=%zu: last guard word written rejected", n));
        expect(rejected([](ScanBufs& x) { x.total.post[1] = 0u; }), fmt("scan n=%zu: total guard written rejected", n));
        expect(rejected([](ScanBufs& x) { x.temp.post[x.temp.words] = 0u; }), fmt("scan n=%zu: workspace guard written rejected", n));
    }

    // sorts: position (in the sorted list) of two neighbours with equal window
    auto equal_pair = [](const SortCase& c, const SortRef& f) -> size_t {
        for (size_t i = 0; i + 1 < f.pos.size(); ++i)
            if (window(c.keys[f.pos[i]], c.begin, c.end) == window(c.keys[f.pos[i + 1]], c.begin, c.end)) return i;
        return (size_t)-1;
    };
    const SortEdit swap_equal = [&](const SortCase& c, SortBufs& b, const SortRef& f) {
        const size_t i = equal_pair(c, f);
        if (i == (size_t)-1) return false;
        Buf& fk = f.in_b ? b.kb : b.ka;
        Buf& fv = f.in_b ? b.vb : b.va;
        std::swap(fv.post[i], fv.post[i + 1]);
        if (!c.planned) std::swap(fk.post[i], fk.post[i + 1]);
        if (c.planned) {   // the gathered rows move with their values: only stability is broken
            std::swap(b.rs.post[2 * i], b.rs.post[2 * i + 2]);
            std::swap(b.rs.post[2 * i + 1], b.rs.post[2 * i + 3]);
            std::swap(b.cnt.post[i], b.cnt.post[i + 1]);
        }
        return true;
    };
    const SortEdit kept_plus = [](const SortCase&, SortBufs& b, const SortRef&) { b.kept.post[0] += 1u; return true; };
    const SortEdit kept_minus = [](const SortCase&, SortBufs& b, const SortRef&) { b.kept.post[0] -= 1u; return true; };
    const SortEdit tail_val = [](const SortCase& c, SortBufs& b, const SortRef& f) {
        if (f.pos.size() >= c.n) return false;
        (f.in_b ? b.vb : b.va).post[f.pos.size()] ^= 1u;
        return true;
    };
    const SortEdit tail_key = [](const SortCase& c, SortBufs& b, const SortRef& f) {
        if (f.pos.size() >= c.n) return false;
        (f.in_b ? b.kb : b.ka).post[c.n - 1] ^= 1u;
        return true;
    };
    auto first_present = [](const SortCase& c, const SortBufs& b) -> size_t {
        for (size_t k = 0; k < c.nranges; ++k)
            if (b.ranges.post[2 * k + 1] != 0u) return k;
        return (size_t)-1;
    };
    const SortEdit range_end = [&](const SortCase& c, SortBufs& b, const SortRef&) {
        const size_t k = first_present(c, b);
        if (k == (size_t)-1) return false;
        b.ranges.post[2 * k + 1] -= 1u;
        return true;
    };
    const SortEdit range_start = [&](const SortCase& c, SortBufs& b, const SortRef&) {
        const size_t k = first_present(c, b);
        if (k == (size_t)-1) return false;
        b.ranges.post[2 * k] += 1u;
        return true;
    };
    const SortEdit range_absent = [](const SortCase& c, SortBufs& b, const SortRef&) {
        for (size_t k = 0; k < c.nranges; ++k)
            if (b.ranges.post[2 * k + 1] == 0u) {
                b.ranges.post[2 * k] = 0u;
                b.ranges.post[2 * k + 1] = 1u;
                return true;
            }
        return false;
    };
    const SortEdit rect_wrong_id = [](const SortCase& c, SortBufs& b, const SortRef& f) {
        // rank i takes the rectangle of another id (one whose rectangle differs)
        for (size_t i = 0; i < f.pos.size(); ++i)
            for (size_t id = 0; id < c.n; ++id)
                if (c.rect[2 * id] != b.rs.post[2 * i] || c.rect[2 * id + 1] != b.rs.post[2 * i + 1]) {
                    b.rs.post[2 * i] = c.rect[2 * id];
                    b.rs.post[2 * i + 1] = c.rect[2 * id + 1];
                    return true;
                }
        return false;
    };
    const SortEdit count_wrong = [](const SortCase&, SortBufs& b, const SortRef& f) {
        if (f.pos.empty()) return false;
        b.cnt.post[f.pos.size() / 2] += 1u;
        return true;
    };
    const SortEdit count_tail = [](const SortCase& c, SortBufs& b, const SortRef& f) {
        if (f.pos.size() >= c.n) return false;
        b.cnt.post[f.pos.size()] = 0u;
        return true;
    };
    const SortEdit plan_flag = [](const SortCase&, SortBufs& b, const SortRef&) { b.temp.post[lsr::RTS_PLAN_OFF / 4 + 1] ^= 1u; return true; };
    const SortEdit plan_base = [](const SortCase&, SortBufs& b, const SortRef&) { b.temp.post[lsr::RTS_PLAN_OFF / 4] += 0x100u; return true; };
    auto guard_edits = [](const SortCase& c) {
        std::vector<std::pair<std::string, SortEdit>> v;
        SortBufs probe = sort_bufs(c);
        const size_t nb = probe.all().size();
        for (size_t j = 0; j < nb; ++j)
            v.emplace_back(std::string("guard word of ") + probe.all()[j]->name + " written",
                           [j](const SortCase&, SortBufs& b, const SortRef&) {
                               Buf* p = b.all()[j];
                               p->post[p->words + (j % GUARD)] ^= 0x10u;
                               return true;
                           });
        return v;
    };

    {   // host plan, one pass (result in b) and two passes (result in a), with dropped keys
        for (int end : {8, 13}) {
            SortCase c = host_case(fmt("host [0,%d) kept", end), 5000, 0, end, P_RANDOM, true, S_TENTH, 7u);
            std::vector<std::pair<std::string, SortEdit>> e = {
                {"two equal-key values swapped", swap_equal}, {"kept one too many", kept_plus}, {"kept one too few", kept_minus},
                {"tail value written", tail_val},             {"tail key written", tail_key}};
            for (auto& g : guard_edits(c)) e.push_back(g);
            selftest_sort(c, e);
        }
    }
    {   // ranges
        SortCase c = ranges_case("ranges nranges=12 keys<16 [0,4) dropped", 3000, 4, 12, 16, 5, true, 9u);
        std::vector<std::pair<std::string, SortEdit>> e = {{"two equal-key values swapped", swap_equal},
                                                           {"range end off by one", range_end},
                                                           {"range start off by one", range_start},
                                                           {"range written for an absent key", range_absent},
                                                           {"kept one too many", kept_plus},
                                                           {"tail value written", tail_val}};
        for (auto& g : guard_edits(c)) e.push_back(g);
        selftest_sort(c, e);
    }
    {   // device plan, both plans
        for (int set : {K_H, K_B}) {
            SortCase c = depth_case("planned", 4000, set, S_TENTH, 13u);
            std::vector<std::pair<std::string, SortEdit>> e = {{"two equal-key values swapped", swap_equal},
                                                               {"kept one too many", kept_plus},
                                                               {"kept one too few", kept_minus},
                                                               {"tail value written", tail_val},
                                                               {"rect_sorted taken from the wrong id", rect_wrong_id},
                                                               {"count wrong", count_wrong},
                                                               {"culled rank's count written", count_tail},
                                                               {"plan flag wrong", plan_flag},
                                                               {"plan kbase wrong", plan_base}};
            if (equal_pair(c, sort_ref(c)) == (size_t)-1) e.erase(e.begin());   // (b) may have no two equal keys
            for (auto& g : guard_edits(c)) e.push_back(g);
            selftest_sort(c, e);
        }
        // the plans the case list names agree with the plan rule on the key sets as generated
        for (int set = K_A; set <= K_H; ++set)
            for (int share = S_NONE; share <= S_ALL; ++share)
                for (size_t n : {(size_t)1, (size_t)64, (size_t)9233}) {
                    const SortCase c = depth_case("planned", n, set, share, 17u + (uint32_t)n);
                    const SortRef f = sort_ref(c);
                    if (c.want_three >= 0 && ((uint32_t)c.want_three != f.three || c.want_kbase != f.kbase))
                        expect(false, c.name + fmt(" n=%zu: named plan == plan rule", n));
                }
        expect(true, "named plans agree with the plan rule");
    }
    {   // an empty segment of a batch: anything written is rejected
        SortCase c = ranges_case("empty segment", 0, 13, 8, 8, 3, true, 19u);
        SortBufs b = sort_bufs(c);
        int ret = 0;
        simulate_sort(c, b, &ret);
        b.kept.post[0] = SENT;   // a skipped segment's kept word is not written
        Report r;
        check_sort(r, c, b, 0);
        expect(r.bad == 0, "empty segment: untouched buffers accepted");
        b.kept.post[0] = 0u;
        Report q;
        g_quiet = true;
        check_sort(q, c, b, 0);
        g_quiet = false;
        expect(q.bad != 0, "empty segment: kept written rejected");
    }
    printf("selftest: %d failed\n", g_self_bad);
    return g_self_bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string g = argc > 1 ? argv[1] : "";
    if (g == "--selftest") return selftest();
    const std::pair<const char*, void (*)()> groups[] = {{"scan", group_scan},           {"scan_batch", group_scan_batch},
                                                         {"host_plan", group_host_plan}, {"ranges", group_ranges},
                                                         {"depth_plan", group_depth_plan}, {"batch", group_batch}};
    for (const auto& e : groups)
        if (g == e.first) {
            const auto t0 = std::chrono::steady_clock::now();
            e.second();
            const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            printf("group %s: %d cases, %d failed, %.1f s\n", e.first, g_cases, g_failed, s);
            return g_failed ? 1 : 0;
        }
    fprintf(stderr, "usage: t_sort_paths <scan|scan_batch|host_plan|ranges|depth_plan|batch> | --selftest\n");
    return 64;
}
