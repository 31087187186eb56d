// fthe_hist.hip -- device-side index work of the homomorphic histogram:
// the CSR of (feature, bin) segments built from dense_bin_id, and the pass
// planner of the segmented K-way product.  Integer bookkeeping only (the
// ciphertext products run in the montprog kernel); everything stays in HBM so
// a level's histogram never round-trips through the host.
//
// Reference loop being replaced (hist_tree_builder.cpp:565-595, :640-664):
//   for fid: for iid in node: bid = dense_bin_id[iid*n_column + fid];
//            if (bid != max_num_bin) hist[cut_col_ptr[fid] + bid] += gh[iid]
// Products mod n^2 commute, so the order of the members inside a segment does
// not change the result; the scatter below is atomic (unordered).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <cstdint>
#include "fthe_glue.h"

namespace fthe {

// thread t = (r, f) over n_sel x n_col, f fastest (one instance's bin row is contiguous)
__device__ __forceinline__ bool hist_key(const uint8_t *__restrict__ bin, int n_col, const int32_t *__restrict__ cut,
                                         int max_bin, const int32_t *__restrict__ inst, size_t t, int64_t &iid,
                                         int64_t &key) {
    const size_t r = t / (size_t)n_col;
    const int f = (int)(t - r * (size_t)n_col);
    iid = inst ? (int64_t)inst[r] : (int64_t)r;
    const int bid = bin[(size_t)iid * n_col + f];
    key = (int64_t)cut[f] + bid;
    return bid != max_bin;
}

__global__ void k_hist_count(const uint8_t *__restrict__ bin, int n_col, const int32_t *__restrict__ cut, int max_bin,
                             const int32_t *__restrict__ inst, size_t n_sel, int planes, int64_t n_bins,
                             unsigned long long *__restrict__ cnt) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_sel * (size_t)n_col) return;
    int64_t iid, key;
    if (!hist_key(bin, n_col, cut, max_bin, inst, t, iid, key)) return;
    for (int p = 0; p < planes; p++) atomicAdd(&cnt[p * n_bins + key], 1ull);
}

__global__ void k_hist_scatter(const uint8_t *__restrict__ bin, int n_col, const int32_t *__restrict__ cut, int max_bin,
                               const int32_t *__restrict__ inst, size_t n_sel, int planes, int64_t n_bins, size_t count,
                               const int64_t *__restrict__ seg, unsigned long long *__restrict__ cursor,
                               int64_t *__restrict__ idx) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_sel * (size_t)n_col) return;
    int64_t iid, key;
    if (!hist_key(bin, n_col, cut, max_bin, inst, t, iid, key)) return;
    for (int p = 0; p < planes; p++) {
        const int64_t s = p * n_bins + key;
        const unsigned long long pos = atomicAdd(&cursor[s], 1ull);
        idx[seg[s] + (int64_t)pos] = iid + (int64_t)p * (int64_t)count;
    }
}

// groups of <= K members per segment (an empty segment still makes one group: the integer 1)
__global__ void k_group_counts(const int64_t *__restrict__ seg, size_t nseg, int K, int64_t *__restrict__ ng) {
    size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > nseg) return;
    if (s == nseg) { ng[s] = 0; return; }
    const int64_t n = seg[s + 1] - seg[s];
    ng[s] = n > K ? (n + K - 1) / K : 1;
}

// gidx[j*G + g] = member j of group g (-1: none); members == nullptr -> identity
__global__ void k_plan_groups(const int64_t *__restrict__ seg, const int64_t *__restrict__ members, size_t nseg,
                              const int64_t *__restrict__ gptr, size_t G, int K, int64_t *__restrict__ gidx) {
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    size_t lo = 0, hi = nseg;                 // largest s with gptr[s] <= g (gptr strictly increasing)
    while (hi - lo > 1) {
        size_t mid = (lo + hi) / 2;
        if (gptr[mid] <= (int64_t)g) lo = mid; else hi = mid;
    }
    const int64_t q = (int64_t)g - gptr[lo];
    const int64_t b = seg[lo] + q * K, e = seg[lo + 1];
    for (int j = 0; j < K; j++) {
        const int64_t t = b + j;
        gidx[(size_t)j * G + g] = t < e ? (members ? members[t] : t) : -1;
    }
}

__global__ void k_u64_to_i64(const unsigned long long *__restrict__ a, int64_t *__restrict__ b, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) b[i] = (int64_t)a[i];
}

// out[0..n) = exclusive prefix sums of in[0..n) (hipcub); tmp grows as needed
int exclusive_scan_i64(const int64_t *in, int64_t *out, size_t n, void *&tmp, size_t &tmp_bytes, hipStream_t st) {
    size_t need = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, n, st) != hipSuccess) return -2;
    if (need > tmp_bytes) {
        if (tmp) hipFree(tmp);
        tmp = nullptr; tmp_bytes = 0;
        if (hipMalloc(&tmp, need) != hipSuccess) return -6;
        tmp_bytes = need;
    }
    return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, in, out, n, st) == hipSuccess ? 0 : -2;
}

// The reference's first `hist[bin] = hist[bin] + gh[iid]` into an unencrypted zero encrypts that zero
// (GHPair::operator+, common.h:156-160), so a populated bin is Enc(0) * prod(members).
// ezm[s] = enc_zero[s] for a populated segment (seg[s+1] > seg[s]) and the integer 1 for an empty
// one, which keeps the reference's unencrypted zero; one thread per word.
__global__ void k_zero_first_rows(const uint32_t *__restrict__ ez, const int64_t *__restrict__ seg, size_t nseg,
                                  int cw, uint32_t *__restrict__ ezm) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nseg * (size_t)cw) return;
    const size_t s = t / (size_t)cw, w = t - s * (size_t)cw;
    ezm[t] = seg[s + 1] > seg[s] ? ez[t] : (uint32_t)(w == 0);
}

// ---------------------------------------------------------------------------
// Per-row plaintext weights (fthe_scalar_mul_rows / fthe_dot_segments): the control of the
// windowed powers and of the bucket (Pippenger) dot product.  Exponents are ew little-endian words per row;
// a window of w = 4 or 8 bits never straddles a word.
__device__ __forceinline__ uint32_t exp_digit(const uint32_t *__restrict__ e, int ew, int j, int w) {
    const int bit0 = j * w, wd = bit0 >> 5;
    return wd < ew ? (e[wd] >> (bit0 & 31)) & ((1u << w) - 1u) : 0u;
}

// *maxbits = max(*maxbits, bit length of the largest exponent); one atomic per block that holds a nonzero one
__global__ void k_exp_maxbits(const uint32_t *__restrict__ e, int ew, size_t count, int *__restrict__ maxbits) {
    __shared__ int sm;
    if (threadIdx.x == 0) sm = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        const uint32_t *r = e + i * (size_t)ew;
        int bits = 0;
        for (int wd = ew - 1; wd >= 0 && !bits; wd--)
            if (r[wd]) bits = 32 * wd + 32 - __clz((int)r[wd]);
        if (bits) atomicMax(&sm, bits);
    }
    __syncthreads();
    if (threadIdx.x == 0 && sm) atomicMax(maxbits, sm);
}

// The gather lists of a chunk of m rows whose table holds x^d at row (d - 1) m + i:
// g[j m + i] = digit j of e[i] ? (digit - 1) m + i : -1 (the integer 1), for the nwin 4-bit windows.
__global__ void k_exp_windows(const uint32_t *__restrict__ e, int ew, size_t m, int nwin, int64_t *__restrict__ g) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t *r = e + i * (size_t)ew;
    for (int j = 0; j < nwin; j++) {
        const uint32_t d = exp_digit(r, ew, j, 4);
        g[(size_t)j * m + i] = d ? (int64_t)((size_t)(d - 1) * m + i) : -1;
    }
}

// out[g] = idx[g] < 0 ? 1 : src[idx[g]] (rows of cw words); one thread per word
__global__ void k_gather_rows(const uint32_t *__restrict__ src, const int64_t *__restrict__ idx, int cw, size_t count,
                              uint32_t *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count * (size_t)cw) return;
    const size_t g = t / (size_t)cw, w = t - g * (size_t)cw;
    const int64_t r = idx[g];
    out[t] = r < 0 ? (uint32_t)(w == 0) : src[(size_t)r * cw + w];
}

// out[0 .. count) = the integer 1
__global__ void k_rows_one(int cw, size_t count, uint32_t *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count * (size_t)cw) out[t] = (uint32_t)(t % (size_t)cw == 0);
}

// *bad = 1 when an index falls outside [0, rows)
__global__ void k_idx_check(const int64_t *__restrict__ idx, size_t n, size_t rows, int *__restrict__ bad) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n && (idx[t] < 0 || (size_t)idx[t] >= rows)) *bad = 1;
}

// Term t of the dot product: its segment s (seg[s] <= t < seg[s + 1], by binary search; empty segments are
// stepped over) and, when s lies in the chunk [s0, s0 + ns), its buckets: digit d != 0 of window j goes to
// bucket ((s - s0) nwin + j) D + (D - d), digits descending inside a (segment, window).
__device__ __forceinline__ bool dot_term(const int64_t *__restrict__ seg, size_t nseg, size_t s0, size_t ns, size_t t,
                                         size_t &s_rel) {
    size_t lo = 0, hi = nseg;                 // smallest s with seg[s + 1] > t
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (seg[mid + 1] > (int64_t)t) hi = mid; else lo = mid + 1;
    }
    if (lo >= nseg || lo < s0 || lo >= s0 + ns) return false;
    s_rel = lo - s0;
    return true;
}

__global__ void k_dot_count(const uint32_t *__restrict__ e, int ew, const int64_t *__restrict__ seg, size_t nseg,
                            size_t terms, size_t s0, size_t ns, int w, int nwin, unsigned long long *__restrict__ cnt) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= terms) return;
    size_t s;
    if (!dot_term(seg, nseg, s0, ns, t, s)) return;
    const uint32_t *r = e + t * (size_t)ew;
    const size_t D = ((size_t)1 << w) - 1;
    for (int j = 0; j < nwin; j++) {
        const uint32_t d = exp_digit(r, ew, j, w);
        if (d) atomicAdd(&cnt[(s * nwin + j) * D + (D - d)], 1ull);
    }
}

__global__ void k_dot_scatter(const uint32_t *__restrict__ e, int ew, const int64_t *__restrict__ seg, size_t nseg,
                              size_t terms, size_t s0, size_t ns, int w, int nwin, const int64_t *__restrict__ idx,
                              const int64_t *__restrict__ bptr, unsigned long long *__restrict__ cursor,
                              int64_t *__restrict__ bidx) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= terms) return;
    size_t s;
    if (!dot_term(seg, nseg, s0, ns, t, s)) return;
    const uint32_t *r = e + t * (size_t)ew;
    const size_t D = ((size_t)1 << w) - 1;
    const int64_t row = idx ? idx[t] : (int64_t)t;
    for (int j = 0; j < nwin; j++) {
        const uint32_t d = exp_digit(r, ew, j, w);
        if (!d) continue;
        const size_t b = (s * nwin + j) * D + (D - d);
        const unsigned long long pos = atomicAdd(&cursor[b], 1ull);
        bidx[bptr[b] + (int64_t)pos] = row;
    }
}

// One pass of the bucket products: of the G planned groups (gidx as k_plan_groups writes it, K lists of G) only
// those with two members or more need products.  They are compacted, in any order, into cg (K lists, G apart,
// *count entries each); where[g] says what group g becomes: a row of the source (>= 0, its only member), the
// integer 1 (-1, no member) or product -where[g] - 2 of the compacted groups.
__global__ void k_dot_active(const int64_t *__restrict__ gidx, size_t G, int K, unsigned long long *__restrict__ count,
                             int64_t *__restrict__ cg, int64_t *__restrict__ where) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    if (gidx[G + g] < 0) { where[g] = gidx[g]; return; }
    const size_t a = (size_t)atomicAdd(count, 1ull);
    for (int j = 0; j < K; j++) cg[(size_t)j * G + a] = gidx[(size_t)j * G + g];
    where[g] = -(int64_t)a - 2;
}

// out[g] = where[g] >= 0 ? src[where[g]] : where[g] == -1 ? 1 : prod[-where[g] - 2]; one thread per word
__global__ void k_gather_rows2(const uint32_t *__restrict__ src, const uint32_t *__restrict__ prod,
                               const int64_t *__restrict__ where, int cw, size_t count, uint32_t *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count * (size_t)cw) return;
    const size_t g = t / (size_t)cw, w = t - g * (size_t)cw;
    const int64_t r = where[g];
    out[t] = r >= 0 ? src[(size_t)r * cw + w] : r == -1 ? (uint32_t)(w == 0) : prod[(size_t)(-r - 2) * cw + w];
}

// yi[i nsj + j ns + s] = (s nwin + j) D + i: position i of every (segment, window)'s buckets, in the plane
// order (window-major) the Horner step reads
__global__ void k_dot_digit_lists(size_t ns, int nwin, int D, int64_t *__restrict__ yi) {
    const size_t nsj = ns * (size_t)nwin;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nsj * (size_t)D) return;
    const size_t i = t / nsj, q = t - i * nsj, j = q / ns, s = q - j * ns;
    yi[t] = (int64_t)((s * nwin + j) * (size_t)D + i);
}

}  // namespace fthe
