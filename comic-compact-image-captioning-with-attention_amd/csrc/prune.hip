// Gradual magnitude pruning (`--prune_sparsity`, Zhu & Gupta 2017): the mask of the flat parameter buffer and the exact
// selection of the weights that go (include/comic_hip.h: comic_prune_select, comic_prune_mask_buffer,
// comic_prune_mask_from_zeros).
//
// The mask is one bit per element of the flat buffer (bit i % 32 of word i / 32, 1 = live).  A mask event prunes, per GROUP
// of segments (one variable, or all prunable variables together), the first k elements of this ordering:
//   already pruned elements first, then the live ones by ascending |w| compared on the IEEE bits of |w| (-0.0 and +0.0 tie,
//   +x and -x tie, denormals order correctly), ties by LOWEST FLAT INDEX.
// Every rank of a data-parallel run has to pick the same weights, so the selection is exact and does not depend on the order
// in which workgroups run: integer histograms only (LDS per workgroup, flushed with integer atomics), no float atomics, no
// sort.  The passes, each over the prunable segments in chunks of kChunk elements:
//   hist x 4 ....... digit-wise descent through the 32-bit key, 8 bits a pass, most significant first: the histogram of the
//                    digit among the live elements whose higher digits equal the prefix found so far (pass 0 also counts the
//                    already pruned elements); `descend` (one thread per group) then picks the digit in which the wanted
//                    rank falls.  After pass 3 the prefix is the threshold key T and the remaining rank is r, the number
//                    of elements equal to T that go.
//   tie_count ...... elements equal to T per chunk;  tie_scan: exclusive prefix over a group's chunks in flat order.
//   apply .......... key < T goes; key == T goes when its rank among the equal ones (chunk base + ballot prefix inside the
//                    chunk) is below r.  A newly pruned element gets its bit cleared (integer atomic AND) and +0.0f in w, m,
//                    v and the shadow.  Nothing else is written: padding and non-prunable elements are in no segment.
// A group whose target is not above its pruned count is inactive after pass 0 and costs nothing more: masks are sticky.
#include <limits.h>

#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr int kThreads = 256;
constexpr int kChunk = 8192;          // elements of a chunk: one workgroup, one group
constexpr int kBins = 256;            // 8 bits a pass; bin kBins counts the already pruned elements (pass 0)
constexpr int kMaxBlocks = 1024;

struct Seg { long first, count, group; };                 // the caller's table: three int64 per segment
struct GroupState { long need; unsigned prefix; int active; };
struct Table { const Seg* segs; int n_seg; int n_groups; long n_total; };
struct ChunkRef { long start; int len; int group; };

// a segment outside the buffer or of an unknown group has no chunks: nothing of it is read or written
__device__ __forceinline__ long seg_chunks(const Table& t, const Seg& s) {
  if (s.first < 0 || s.count <= 0 || s.count > t.n_total || s.first > t.n_total - s.count || s.group < 0 ||
      s.group >= t.n_groups)
    return 0;
  return (s.count + kChunk - 1) / kChunk;
}
// chunk c of the table, counted through the segments in their order
__device__ __forceinline__ bool locate(const Table& t, long c, ChunkRef& r) {
  for (int s = 0; s < t.n_seg; ++s) {
    const Seg sg = t.segs[s];
    const long nc = seg_chunks(t, sg);
    if (c < nc) {
      r.start = sg.first + c * kChunk;
      r.len = (int)min((long)kChunk, sg.count - c * kChunk);
      r.group = (int)sg.group;
      return true;
    }
    c -= nc;
  }
  return false;
}
__device__ __forceinline__ bool live_bit(const uint32_t* mask, long a) { return (mask[a >> 5] >> (a & 31)) & 1u; }
__device__ __forceinline__ unsigned key_of(float x) { return __float_as_uint(x) & 0x7FFFFFFFu; }

__global__ __launch_bounds__(kThreads) void prune_hist_kernel(const float* __restrict__ w, const uint32_t* __restrict__ mask,
                                                              Table t, long chunk_cap, const GroupState* __restrict__ st,
                                                              u64* __restrict__ hist, int pass) {
  __shared__ unsigned h[kBins + 1];
  const int tid = threadIdx.x, shift = 24 - 8 * pass;
  for (long c = blockIdx.x; c < chunk_cap; c += gridDim.x) {
    ChunkRef r;
    if (!locate(t, c, r)) break;                              // (uniform: c is the workgroup's)
    if (pass > 0 && !st[r.group].active) continue;
    const unsigned prefix = pass > 0 ? st[r.group].prefix : 0u;
    for (int i = tid; i <= kBins; i += kThreads) h[i] = 0u;
    __syncthreads();
    for (int i = tid; i < r.len; i += kThreads) {
      const long a = r.start + i;
      if (!live_bit(mask, a)) {
        if (pass == 0) atomicAdd(&h[kBins], 1u);
        continue;
      }
      const unsigned key = key_of(w[a]);
      if (pass > 0 && (key >> (shift + 8)) != (prefix >> (shift + 8))) continue;
      atomicAdd(&h[(key >> shift) & (kBins - 1)], 1u);
    }
    __syncthreads();
    for (int i = tid; i <= kBins; i += kThreads)
      if (h[i]) atomicAdd(&hist[(long)r.group * (kBins + 1) + i], (u64)h[i]);
    __syncthreads();
  }
}

// one thread per group: the digit in which rank `need` falls; the histogram is cleared for the next pass
__global__ void prune_descend_kernel(GroupState* __restrict__ st, u64* __restrict__ hist, const long* __restrict__ k,
                                     int n_groups, int pass) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  u64* h = hist + (long)g * (kBins + 1);
  GroupState s = st[g];
  if (pass == 0) {
    u64 live = 0;
    for (int d = 0; d < kBins; ++d) live += h[d];
    const long pruned = (long)h[kBins], total = (long)live + pruned;
    s.need = min(k[g], total) - pruned;                       // <= 0: the target is reached already (masks are sticky)
    s.prefix = 0u;
    s.active = s.need > 0 ? 1 : 0;
  }
  if (s.active) {
    u64 below = 0;
    int d = 0;
    for (; d < kBins - 1; ++d) {
      if (below + h[d] >= (u64)s.need) break;
      below += h[d];
    }
    s.need -= (long)below;
    s.prefix |= (unsigned)d << (24 - 8 * pass);
  }
  for (int d = 0; d <= kBins; ++d) h[d] = 0;
  st[g] = s;
}

__global__ __launch_bounds__(kThreads) void prune_tie_count_kernel(const float* __restrict__ w,
                                                                   const uint32_t* __restrict__ mask, Table t, long chunk_cap,
                                                                   const GroupState* __restrict__ st,
                                                                   unsigned* __restrict__ cnt) {
  __shared__ unsigned total;
  const int tid = threadIdx.x;
  for (long c = blockIdx.x; c < chunk_cap; c += gridDim.x) {
    ChunkRef r;
    if (!locate(t, c, r)) break;
    const GroupState s = st[r.group];
    if (!s.active) continue;                                  // (cnt[c] stays 0: the workspace was cleared)
    if (tid == 0) total = 0u;
    __syncthreads();
    unsigned mine = 0;
    for (int i = tid; i < r.len; i += kThreads) {
      const long a = r.start + i;
      mine += (live_bit(mask, a) && key_of(w[a]) == s.prefix) ? 1u : 0u;
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (tid == 0) cnt[c] = total;
    __syncthreads();
  }
}

// one workgroup per group: base[c] = elements equal to T in the group's chunks before chunk c, in flat order
__global__ __launch_bounds__(kThreads) void prune_tie_scan_kernel(Table t, long chunk_cap, const GroupState* __restrict__ st,
                                                                  const unsigned* __restrict__ cnt, long* __restrict__ base) {
  __shared__ long sc[kThreads];
  const int g = blockIdx.x, tid = threadIdx.x;
  if (!st[g].active) return;
  long total = 0;
  for (int s = 0; s < t.n_seg; ++s) total += seg_chunks(t, t.segs[s]);
  total = min(total, chunk_cap);
  long carry = 0;
  for (long c0 = 0; c0 < total; c0 += kThreads) {
    const long c = c0 + tid;
    ChunkRef r;
    const bool mine = c < total && locate(t, c, r) && r.group == g;
    const long x = mine ? (long)cnt[c] : 0;
    sc[tid] = x;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {                  // inclusive scan of the tile
      const long y = tid >= d ? sc[tid - d] : 0;
      __syncthreads();
      sc[tid] += y;
      __syncthreads();
    }
    if (mine) base[c] = carry + sc[tid] - x;
    carry += sc[kThreads - 1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void prune_apply_kernel(float* __restrict__ w, uint32_t* mask, Table t, long chunk_cap,
                                                               const GroupState* __restrict__ st,
                                                               const long* __restrict__ base, float* __restrict__ m,
                                                               float* __restrict__ v, float* __restrict__ shadow) {
  __shared__ unsigned wcnt[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (long c = blockIdx.x; c < chunk_cap; c += gridDim.x) {
    ChunkRef r;
    if (!locate(t, c, r)) break;
    const GroupState s = st[r.group];
    if (!s.active) continue;
    long seen = base[c];                                      // equal elements of the group in front of this round
    for (int i0 = 0; i0 < r.len; i0 += kThreads) {
      const int i = i0 + tid;
      const long a = r.start + i;
      const bool live = i < r.len && live_bit(mask, a);
      const unsigned key = live ? key_of(w[a]) : 0u;
      const bool eq = live && key == s.prefix;
      const u64 bal = __ballot(eq);
      if (lane == 0) wcnt[wave] = (unsigned)__popcll(bal);
      __syncthreads();
      unsigned before = 0, all = 0;
      for (int k = 0; k < kThreads / 64; ++k) {
        before += k < wave ? wcnt[k] : 0u;
        all += wcnt[k];
      }
      const long rank = seen + before + __popcll(bal & ((1ull << lane) - 1ull));
      if (live && (key < s.prefix || (eq && rank < s.need))) {
        atomicAnd(&mask[a >> 5], ~(1u << (a & 31)));
        w[a] = 0.f;
        m[a] = 0.f;
        v[a] = 0.f;
        if (shadow) shadow[a] = 0.f;
      }
      seen += all;
      __syncthreads();
    }
  }
}

__global__ void prune_mask_buffer_kernel(float* __restrict__ x, const uint32_t* __restrict__ mask, long first_bit, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!live_bit(mask, first_bit + i)) x[i] = 0.f;
}

__global__ __launch_bounds__(kThreads) void prune_mask_from_zeros_kernel(const float* __restrict__ w, uint32_t* mask, Table t,
                                                                         long chunk_cap) {
  for (long c = blockIdx.x; c < chunk_cap; c += gridDim.x) {
    ChunkRef r;
    if (!locate(t, c, r)) break;
    for (int i = threadIdx.x; i < r.len; i += kThreads) {
      const long a = r.start + i;
      if (w[a] == 0.f) atomicAnd(&mask[a >> 5], ~(1u << (a & 31)));
    }
  }
}

inline int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }
inline int64_t chunk_cap_of(int64_t n_total, int n_seg) { return n_total / kChunk + n_seg; }
struct Layout { int64_t st, hist, cnt, base, bytes; };
inline Layout layout_of(int64_t n_total, int n_seg, int n_groups) {
  Layout l;
  const int64_t cap = chunk_cap_of(n_total, n_seg);
  l.st = 0;
  l.hist = l.st + align256((int64_t)n_groups * (int64_t)sizeof(GroupState));
  l.cnt = l.hist + align256((int64_t)n_groups * (kBins + 1) * (int64_t)sizeof(u64));
  l.base = l.cnt + align256(cap * (int64_t)sizeof(unsigned));
  l.bytes = l.base + align256(cap * (int64_t)sizeof(long));
  return l;
}
inline bool table_ok(int64_t n_total, int n_seg, int n_groups) {
  return n_total > 0 && n_seg > 0 && n_seg <= 4096 && n_groups > 0 && n_groups <= n_seg;
}

}  // namespace

extern "C" int64_t comic_prune_workspace_bytes(int64_t n_total, int n_seg, int n_groups) {
  if (!table_ok(n_total, n_seg, n_groups)) return -1;
  return layout_of(n_total, n_seg, n_groups).bytes;
}

extern "C" int comic_prune_select(float* w, uint32_t* mask, int64_t n_total, const int64_t* segments, int n_seg,
                                  const int64_t* targets, int n_groups, float* m, float* v, float* shadow, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  COMIC_REQUIRE(w && mask && segments && targets && m && v && workspace, "prune_select: null pointer");
  COMIC_REQUIRE(table_ok(n_total, n_seg, n_groups), "prune_select: bad table (n_total %lld, %d segments, %d groups)",
                (long long)n_total, n_seg, n_groups);
  static_assert(sizeof(Seg) == 3 * sizeof(int64_t) && sizeof(GroupState) == 16, "records");
  const Layout l = layout_of(n_total, n_seg, n_groups);
  COMIC_REQUIRE(workspace_bytes >= l.bytes, "prune_select: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)l.bytes);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  GroupState* st = (GroupState*)(ws + l.st);
  u64* hist = (u64*)(ws + l.hist);
  unsigned* cnt = (unsigned*)(ws + l.cnt);
  long* base = (long*)(ws + l.base);
  if (hipMemsetAsync(workspace, 0, (size_t)l.bytes, s) != hipSuccess) {
    comic_set_error("prune_select: clearing the workspace failed");
    return 1;
  }
  const Table t = {(const Seg*)segments, n_seg, n_groups, (long)n_total};
  const long cap = (long)chunk_cap_of(n_total, n_seg);
  const dim3 grid((unsigned)(cap < kMaxBlocks ? cap : kMaxBlocks)), block(kThreads);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(prune_hist_kernel, grid, block, 0, s, (const float*)w, (const uint32_t*)mask, t, cap,
                       (const GroupState*)st, hist, pass);
    hipLaunchKernelGGL(prune_descend_kernel, dim3((unsigned)cdiv(n_groups, 64)), dim3(64), 0, s, st, hist,
                       (const long*)targets, n_groups, pass);
  }
  hipLaunchKernelGGL(prune_tie_count_kernel, grid, block, 0, s, (const float*)w, (const uint32_t*)mask, t, cap,
                     (const GroupState*)st, cnt);
  hipLaunchKernelGGL(prune_tie_scan_kernel, dim3((unsigned)n_groups), block, 0, s, t, cap, (const GroupState*)st,
                     (const unsigned*)cnt, base);
  hipLaunchKernelGGL(prune_apply_kernel, grid, block, 0, s, w, mask, t, cap, (const GroupState*)st, (const long*)base, m, v,
                     shadow);
  COMIC_LAUNCH_CHECK("prune_select");
  return 0;
}

extern "C" int comic_prune_mask_buffer(float* x, const uint32_t* mask, int64_t first_bit, int64_t n, void* stream) {
  COMIC_REQUIRE(x && mask && first_bit >= 0 && n > 0, "prune_mask_buffer: null pointer, negative first bit or no elements");
  hipLaunchKernelGGL(prune_mask_buffer_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream, x, mask,
                     (long)first_bit, (long)n);
  COMIC_LAUNCH_CHECK("prune_mask_buffer");
  return 0;
}

extern "C" int comic_prune_mask_from_zeros(const float* w, uint32_t* mask, int64_t n_total, const int64_t* segments,
                                           int n_seg, void* stream) {
  COMIC_REQUIRE(w && mask && segments && n_total > 0 && n_seg > 0 && n_seg <= 4096, "prune_mask_from_zeros: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(mask, 0xFF, (size_t)cdiv64(n_total, 32) * sizeof(uint32_t), s) != hipSuccess) {
    comic_set_error("prune_mask_from_zeros: setting the mask failed");
    return 1;
  }
  const Table t = {(const Seg*)segments, n_seg, INT_MAX, (long)n_total};       // (the groups of the table are not read)
  const long cap = (long)chunk_cap_of(n_total, n_seg);
  hipLaunchKernelGGL(prune_mask_from_zeros_kernel, dim3((unsigned)(cap < kMaxBlocks ? cap : kMaxBlocks)), dim3(kThreads), 0, s,
                     w, mask, t, cap);
  COMIC_LAUNCH_CHECK("prune_mask_from_zeros");
  return 0;
}
