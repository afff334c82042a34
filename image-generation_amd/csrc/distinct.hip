// The equivalence classes of bit-packed spin rows under equality on the spins < n ("DVG distinct v1", include/dvg.h): which
// rows are the same state and how often each state occurs, exactly.  An open-addressing table of row indices in the workspace
// (int32 slots, a power of two >= 2 T of them, no stored hash: every match is a full comparison of the two rows from the
// read-only input); a row is held by a group of lanes that load 16 bytes each.  A slot's class never changes once it is set
// and every row of a class walks the same probe sequence, so a class ends in exactly one slot, which atomicMin leaves holding
// the class's smallest row index whatever the arrival order.  Everything after the insert runs in separate stream-ordered
// launches -- first[] and the class sizes, the flags first[t] == t compacted in order by block sums, a scan of the sums and
// apply, as population.hip does it -- and reads what the launch before it wrote: no thread spins or waits for another thread
// or workgroup, every probe loop is bounded by the capacity.
#include "common.h"
#include "packed_rows.h"

namespace dvg {

constexpr int DS_THREADS = 256;                 // four waves
constexpr int DS_ITEMS = 4;                     // consecutive elements per thread of a scan
constexpr int DS_TILE = DS_THREADS * DS_ITEMS;  // elements per workgroup of a scan
constexpr int DS_MAX_LEVELS = 4;                // 1024^4 > 2^31 rows
constexpr int32_t DS_EMPTY = -1;                // a slot no row has claimed (row indices are >= 0)

// ---------------------------------------------------------------- rows: 16-byte chunks, the pad bits cleared
// Chunk c of a row: its words 4 c .. 4 c + 3, the last word of the row under `tail` (the spins < n), words >= W as 0.  VEC: the
// row starts at a multiple of 16 bytes; a whole chunk is then one 16-byte load.  A partial last chunk is read word by word: the
// words behind W may lie beyond the last row.
template <bool VEC>
__device__ __forceinline__ uint4 ds_chunk(const uint32_t* row, int c, int W, uint32_t tail) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  const int w0 = 4 * c;
  if (w0 + 4 <= W) {
    if (VEC) {
      v = *reinterpret_cast<const uint4*>(row + w0);
    } else {
      v.x = row[w0];
      v.y = row[w0 + 1];
      v.z = row[w0 + 2];
      v.w = row[w0 + 3];
    }
  } else {
    if (w0 < W) v.x = row[w0];
    if (w0 + 1 < W) v.y = row[w0 + 1];
    if (w0 + 2 < W) v.z = row[w0 + 2];
  }
  const int last = W - 1 - w0;
  if (last == 0) v.x &= tail;
  else if (last == 1) v.y &= tail;
  else if (last == 2) v.z &= tail;
  else if (last == 3) v.w &= tail;
  return v;
}

__device__ __forceinline__ uint32_t ds_mix(uint32_t x) {  // the 32-bit finaliser of MurmurHash3
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

// A chunk's share of the row's hash: the words mixed with their positions, summed (so the lanes' shares add in any order).
__device__ __forceinline__ uint32_t ds_hash_chunk(uint4 v, int c) {
  const uint32_t p = 0x9e3779b9u * (uint32_t)(4 * c + 1);
  return ds_mix(v.x + p) + ds_mix(v.y + p + 0x9e3779b9u) + ds_mix(v.z + p + 2u * 0x9e3779b9u) + ds_mix(v.w + p + 3u * 0x9e3779b9u);
}

__device__ __forceinline__ bool ds_ne(uint4 a, uint4 b) { return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) != 0u; }

// What a group of LPR = 2^lpr_log2 lanes (gl the lane's place in it) holds of its row: the chunks gl, gl + LPR, ..; the first
// one stays in registers.  Every function here is called by all 64 lanes of the wave; a lane without a row passes null.
template <bool VEC>
struct DsRow {
  const uint32_t* row;
  uint4 mine;
  uint32_t hash;  // of the whole row, the same in every lane of the group
  __device__ __forceinline__ void load(const uint32_t* r, int gl, int lpr_log2, int chunks, int W, uint32_t tail, uint32_t hash_mask) {
    row = r;
    mine = make_uint4(0u, 0u, 0u, 0u);
    uint32_t h = 0u;
    const int LPR = 1 << lpr_log2;
    if (row) {
      for (int c = gl; c < chunks; c += LPR) {
        const uint4 v = ds_chunk<VEC>(row, c, W, tail);
        if (c == gl) mine = v;
        h += ds_hash_chunk(v, c);
      }
    }
    for (int o = 1; o < LPR; o <<= 1) h += __shfl_xor(h, o);
    hash = ds_mix(h) & hash_mask;
  }
  // this lane's chunks differ from those of `other` (a row of a set with the same W; VO: its 16-byte alignment)
  template <bool VO>
  __device__ __forceinline__ bool differs(const uint32_t* other, int gl, int lpr_log2, int chunks, int W, uint32_t tail) const {
    const int LPR = 1 << lpr_log2;
    bool ne = false;
    for (int c = gl; c < chunks && !ne; c += LPR) {
      const uint4 a = c == gl ? mine : ds_chunk<VEC>(row, c, W, tail);
      ne = ds_ne(a, ds_chunk<VO>(other, c, W, tail));
    }
    return ne;
  }
};

// the lanes of this lane's group, as a mask of the wave
__device__ __forceinline__ unsigned long long ds_group_mask(int lane, int lpr_log2) {
  const int LPR = 1 << lpr_log2;
  return (LPR == 64 ? ~0ull : ((1ull << LPR) - 1ull)) << (lane & ~(LPR - 1));
}

// ---------------------------------------------------------------- fill, insert, first
__global__ __launch_bounds__(DS_THREADS) void distinct_fill_kernel(int32_t* __restrict__ table, uint64_t cap, int32_t* __restrict__ cnt,
                                                                   int64_t T, int32_t* __restrict__ err) {
  const uint64_t stride = (uint64_t)gridDim.x * DS_THREADS;
  const uint64_t i0 = (uint64_t)blockIdx.x * DS_THREADS + threadIdx.x;
  for (uint64_t i = i0; i < cap; i += stride) table[i] = DS_EMPTY;
  for (uint64_t i = i0; i < (uint64_t)T; i += stride) cnt[i] = 0;
  if (i0 == 0) *err = 0;
}

// Row t = g rows + r of the pooled set, one per group of lanes: claim the first EMPTY slot of the probe sequence, or stop at the
// first slot that holds a row equal to this one and lower it to min(slot, t).  slot_of[t]: where the row's class lives.
template <bool VEC>
__global__ __launch_bounds__(DS_THREADS) void distinct_insert_kernel(const uint32_t* __restrict__ bits, int64_t T, int64_t rows,
                                                                     int64_t row_stride, int64_t groups, int64_t group_stride, int W,
                                                                     uint32_t tail, int lpr_log2, uint32_t hash_mask,
                                                                     int32_t* __restrict__ table, uint64_t cap_mask,
                                                                     uint32_t* __restrict__ slot_of, int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63, gl = lane & ((1 << lpr_log2) - 1), chunks = (W + 3) >> 2;
  const int64_t t = ((int64_t)blockIdx.x * DS_THREADS + threadIdx.x) >> lpr_log2;
  const unsigned long long gmask = ds_group_mask(lane, lpr_log2);
  DsRow<VEC> me;
  me.load(packed_row(bits, t, T, rows, row_stride, groups, group_stride), gl, lpr_log2, chunks, W, tail, hash_mask);
  uint64_t slot = (uint64_t)me.hash & cap_mask;
  bool active = me.row != nullptr;
  for (uint64_t probe = 0; probe <= cap_mask; ++probe) {  // (wave-uniform: the groups that are done idle)
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
    int32_t held = DS_EMPTY;
    if (active && gl == 0) held = atomicCAS(&table[slot], DS_EMPTY, (int32_t)t);
    held = __shfl(held, lane & ~((1 << lpr_log2) - 1));
    bool ne = false;
    if (active && held != DS_EMPTY)
      ne = me.template differs<VEC>(packed_row(bits, (int64_t)held, T, rows, row_stride, groups, group_stride), gl, lpr_log2, chunks, W,
                                    tail);
    const bool differ = (__builtin_amdgcn_ballot_w64(ne) & gmask) != 0ull;
    if (active) {
      if (held == DS_EMPTY || !differ) {
        if (gl == 0) {
          if (held != DS_EMPTY && (int64_t)held > t) atomicMin(&table[slot], (int32_t)t);
          slot_of[t] = (uint32_t)slot;
        }
        active = false;
      } else {
        slot = (slot + 1) & cap_mask;
      }
    }
  }
  if (active && gl == 0) *err = 1;  // the table was full: cannot happen at load <= 0.5
}

// first[t] = what the class's slot holds now that every insert is done; the class sizes onto cnt[first]
__global__ __launch_bounds__(DS_THREADS) void distinct_first_kernel(const int32_t* __restrict__ table, const uint32_t* __restrict__ slot_of,
                                                                    int64_t T, int32_t* __restrict__ first_ws, int32_t* __restrict__ first,
                                                                    int32_t* __restrict__ cnt, const int32_t* __restrict__ err) {
  if (*err) return;
  const int64_t t = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
  if (t >= T) return;
  const int32_t f = table[slot_of[t]];
  first_ws[t] = f;
  if (first) first[t] = f;
  atomicAdd(&cnt[f], 1);
}

// ---------------------------------------------------------------- the ordered compaction of the flags first[t] == t
// FLAGS: element i is first[i] == i, else in[i]
template <bool FLAGS>
__device__ __forceinline__ int32_t ds_value(const int32_t* in, int64_t i, int64_t n) {
  if (i >= n) return 0;
  return FLAGS ? (int32_t)((int64_t)in[i] == i) : in[i];
}

// Inclusive scan of the workgroup's DS_TILE values, DS_ITEMS consecutive ones per thread; returns the workgroup's total.
__device__ __forceinline__ int32_t ds_block_scan(int32_t (&k)[DS_ITEMS], int32_t* red) {
#pragma unroll
  for (int i = 1; i < DS_ITEMS; ++i) k[i] += k[i - 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t incl = k[DS_ITEMS - 1];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == 63) red[wave] = incl;
  __syncthreads();
  int32_t before = incl - k[DS_ITEMS - 1], total = 0;
#pragma unroll
  for (int w = 0; w < DS_THREADS / 64; ++w) {
    if (w < wave) before += red[w];
    total += red[w];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < DS_ITEMS; ++i) k[i] += before;
  return total;
}

// SUMS: the block's total into bsum[block].  Otherwise: the exclusive prefix sums of the block's elements, its offset
// boff[block] added (boff null: one block, offset 0), into out; and the total of everything into n_distinct where given.
template <bool FLAGS, bool SUMS>
__global__ __launch_bounds__(DS_THREADS) void distinct_scan_kernel(const int32_t* __restrict__ in, int64_t n, int32_t* __restrict__ bsum,
                                                                   const int32_t* __restrict__ boff, int32_t* __restrict__ out,
                                                                   int64_t* __restrict__ n_distinct, const int32_t* __restrict__ err) {
  __shared__ int32_t red[DS_THREADS / 64];
  const int bad = *err;
  const int64_t i0 = (int64_t)blockIdx.x * DS_TILE + threadIdx.x * DS_ITEMS;
  int32_t k[DS_ITEMS], own[DS_ITEMS];
#pragma unroll
  for (int i = 0; i < DS_ITEMS; ++i) own[i] = k[i] = bad ? 0 : ds_value<FLAGS>(in, i0 + i, n);
  const int32_t total = ds_block_scan(k, red);
  if (SUMS) {
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
  } else {
    const int32_t off = boff ? boff[blockIdx.x] : 0;
#pragma unroll
    for (int i = 0; i < DS_ITEMS; ++i)
      if (i0 + i < n) out[i0 + i] = k[i] - own[i] + off;
    if (n_distinct && threadIdx.x == 0) n_distinct[0] = bad ? -1 : (int64_t)total;
  }
}

// pos[t] = the number of first occurrences before t: class d = pos[first[t]]
__global__ __launch_bounds__(DS_THREADS) void distinct_emit_kernel(const int32_t* __restrict__ first_ws, const int32_t* __restrict__ pos,
                                                                   const int32_t* __restrict__ cnt, int64_t T, int32_t* __restrict__ id,
                                                                   int32_t* __restrict__ rep, int64_t* __restrict__ count,
                                                                   int64_t* __restrict__ other_hits, const int32_t* __restrict__ err) {
  if (*err) return;
  const int64_t t = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
  if (t >= T) return;
  const int32_t f = first_ws[t];
  const int32_t d = pos[f];
  if (id) id[t] = d;
  if ((int64_t)f == t) {
    if (rep) rep[d] = (int32_t)t;
    if (count) count[d] = (int64_t)cnt[t];
    if (other_hits) other_hits[d] = 0;
  }
}

// ---------------------------------------------------------------- the rows of `other`: looked up, never inserted
template <bool VEC>
__global__ __launch_bounds__(DS_THREADS) void distinct_lookup_kernel(const uint32_t* __restrict__ other, int64_t rows_other,
                                                                     int64_t other_row_stride, const uint32_t* __restrict__ bits, int64_t T,
                                                                     int64_t rows, int64_t row_stride, int64_t groups,
                                                                     int64_t group_stride, int W, uint32_t tail, int lpr_log2,
                                                                     uint32_t hash_mask, const int32_t* __restrict__ table,
                                                                     uint64_t cap_mask, const int32_t* __restrict__ pos,
                                                                     int32_t* __restrict__ other_id, int64_t* __restrict__ other_hits,
                                                                     const int32_t* __restrict__ err) {
  if (*err) return;
  const int lane = threadIdx.x & 63, gl = lane & ((1 << lpr_log2) - 1), chunks = (W + 3) >> 2;
  const int64_t u = ((int64_t)blockIdx.x * DS_THREADS + threadIdx.x) >> lpr_log2;
  const unsigned long long gmask = ds_group_mask(lane, lpr_log2);
  DsRow<VEC> me;
  me.load(packed_row(other, u, rows_other, rows_other, other_row_stride, 1, 0), gl, lpr_log2, chunks, W, tail, hash_mask);
  uint64_t slot = (uint64_t)me.hash & cap_mask;
  bool active = me.row != nullptr;
  int32_t found = -1;
  for (uint64_t probe = 0; probe <= cap_mask; ++probe) {
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
    const int32_t held = active ? table[slot] : DS_EMPTY;  // (the same address in every lane of the group)
    bool ne = false;
    if (active && held != DS_EMPTY)
      ne = me.template differs<VEC>(packed_row(bits, (int64_t)held, T, rows, row_stride, groups, group_stride), gl, lpr_log2, chunks, W,
                                    tail);
    const bool differ = (__builtin_amdgcn_ballot_w64(ne) & gmask) != 0ull;
    if (active) {
      if (held == DS_EMPTY) {
        active = false;
      } else if (!differ) {
        found = pos[held];  // the slot holds its class's first row
        active = false;
      } else {
        slot = (slot + 1) & cap_mask;
      }
    }
  }
  if (me.row && gl == 0) {
    if (other_id) other_id[u] = found;
    if (other_hits && found >= 0) atomicAdd(reinterpret_cast<unsigned long long*>(other_hits + found), 1ull);
  }
}

// ---------------------------------------------------------------- host
struct DsLayout {
  uint64_t cap;                     // slots of the table: the power of two >= 2 T
  int levels;                       // scan levels above the flags: level l holds the block sums of level l - 1
  int64_t level_n[DS_MAX_LEVELS];   // elements of level l (level 0: the T flags)
  size_t table, slot_of, first, cnt, pos, sums, err, bytes;  // offsets in int32 units; sums: bsum and boff of every level
};

static DsLayout ds_layout(int64_t T) {
  DsLayout L{};
  L.cap = 2;
  while (L.cap < 2 * (uint64_t)T) L.cap <<= 1;
  size_t sums = 0;
  L.level_n[0] = T;
  L.levels = 0;
  while (L.level_n[L.levels] > DS_TILE) {
    L.level_n[L.levels + 1] = ceil_div(L.level_n[L.levels], DS_TILE);
    ++L.levels;
    sums += 2 * (size_t)L.level_n[L.levels];
  }
  L.table = 0;
  L.slot_of = L.table + (size_t)L.cap;
  L.first = L.slot_of + (size_t)T;
  L.cnt = L.first + (size_t)T;
  L.pos = L.cnt + (size_t)T;
  L.sums = L.pos + (size_t)T;
  L.err = L.sums + sums;
  L.bytes = align_up(sizeof(int32_t) * (L.err + 1), 256);
  return L;
}

// lanes per row (log2): a lane per 16-byte chunk, a wave at the most
static int ds_lpr_log2(int W) {
  const int chunks = (W + 3) / 4;
  int l = 0;
  while (l < 6 && (1 << l) < chunks) ++l;
  return l;
}

static bool ds_rows_vec(const uint32_t* p, int64_t row_stride, int64_t groups, int64_t group_stride) {
  return (uintptr_t)p % 16 == 0 && row_stride % 4 == 0 && (groups == 1 || group_stride % 4 == 0);
}

}  // namespace dvg

using namespace dvg;

extern "C" size_t dvg_packed_distinct_workspace_bytes(int64_t rows, int64_t groups, int n) {
  if (rows < 1 || groups < 1 || n < 1 || (__int128)rows * groups >= ((__int128)1 << 31)) return 0;
  return ds_layout(rows * groups).bytes;
}

extern "C" int dvg_packed_distinct(const uint32_t* bits, int64_t rows, int64_t row_stride, int64_t groups, int64_t group_stride, int n,
                                   const uint32_t* other, int64_t rows_other, int64_t other_row_stride, int32_t* first, int32_t* id,
                                   int32_t* rep, int64_t* count, int64_t* n_distinct, int32_t* other_id, int64_t* other_hits, void* ws,
                                   size_t ws_bytes, dvg_stream_t stream) {
  DVG_REQUIRE(bits, "packed_distinct: bits is null");
  DVG_REQUIRE(n_distinct, "packed_distinct: n_distinct is null");
  DVG_REQUIRE(ws, "packed_distinct: ws is null");
  DVG_REQUIRE((uintptr_t)ws % 4 == 0, "packed_distinct: ws is not aligned to 4 bytes");
  DVG_REQUIRE(n >= 1, "packed_distinct: n=%d must be at least 1", n);
  const int64_t W = ((int64_t)n + 31) / 32;
  DVG_TRY(check_row_geometry("packed_distinct", rows, groups, row_stride, W, group_stride));
  if (other) {
    DVG_REQUIRE(rows_other >= 1, "packed_distinct: rows_other=%lld must be at least 1", (long long)rows_other);
    DVG_REQUIRE(other_row_stride >= W, "packed_distinct: other_row_stride=%lld is less than the %lld words of a row",
                (long long)other_row_stride, (long long)W);
  } else {
    DVG_REQUIRE(!other_id, "packed_distinct: other_id is given without other");
    DVG_REQUIRE(!other_hits, "packed_distinct: other_hits is given without other");
  }
  if ((__int128)groups * rows >= ((__int128)1 << 31)) {
    set_error("packed_distinct: groups=%lld x rows=%lld rows must be below 2^31 (a row index is an int32)", (long long)groups,
              (long long)rows);
    return DVG_E_UNSUPPORTED;
  }
  if (other && rows_other >= ((int64_t)1 << 31)) {
    set_error("packed_distinct: rows_other=%lld must be below 2^31 (a row index is an int32)", (long long)rows_other);
    return DVG_E_UNSUPPORTED;
  }
  const int64_t T = groups * rows;
  const DsLayout L = ds_layout(T);
  if (ws_bytes < L.bytes) {
    set_error("packed_distinct: workspace %zu < %zu", ws_bytes, L.bytes);
    return DVG_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  int32_t* base = (int32_t*)ws;
  int32_t* table = base + L.table;
  uint32_t* slot_of = (uint32_t*)(base + L.slot_of);
  int32_t* first_ws = base + L.first;
  int32_t* cnt = base + L.cnt;
  int32_t* pos = base + L.pos;
  int32_t* err = base + L.err;
  const uint64_t cap_mask = L.cap - 1;
  const int Wi = (int)W, lpr_log2 = ds_lpr_log2(Wi);
  const uint32_t tail = n % 32 ? (1u << (n % 32)) - 1u : 0xFFFFFFFFu;
  const int64_t k = opt(OPT_DISTINCT_HASH_BITS);
  const uint32_t hash_mask = k < 0 || k >= 32 ? 0xFFFFFFFFu : (1u << k) - 1u;
  const dim3 block(DS_THREADS);
  const dim3 per_row((unsigned)ceil_div(T, DS_THREADS));
  const dim3 per_group((unsigned)ceil_div(T << lpr_log2, DS_THREADS));
  const bool vec = ds_rows_vec(bits, row_stride, groups, group_stride);

  const uint64_t fill_blocks = ceil_div((int64_t)L.cap, DS_THREADS);
  DVG_LAUNCH(K_GRBM_SUFFSTATS, distinct_fill_kernel, dim3((unsigned)(fill_blocks < 4096 ? fill_blocks : 4096)), block, 0, s, table, L.cap, cnt,
             T, err);
  if (vec)
    DVG_LAUNCH(K_GRBM_SUFFSTATS, distinct_insert_kernel<true>, per_group, block, 0, s, bits, T, rows, row_stride, groups, group_stride, Wi,
               tail, lpr_log2, hash_mask, table, cap_mask, slot_of, err);
  else
    DVG_LAUNCH(K_GRBM_SUFFSTATS, distinct_insert_kernel<false>, per_group, block, 0, s, bits, T, rows, row_stride, groups, group_stride, Wi,
               tail, lpr_log2, hash_mask, table, cap_mask, slot_of, err);
  DVG_LAUNCH(K_GRBM_SUFFSTATS, distinct_first_kernel, per_row, block, 0, s, (const int32_t*)table, (const uint32_t*)slot_of, T, first_ws,
             first, cnt, (const int32_t*)err);

  // block sums up the levels, the top level in one workgroup, offsets back down: pos = the exclusive scan of the flags
  int32_t* bsum[DS_MAX_LEVELS + 1] = {nullptr};
  int32_t* boff[DS_MAX_LEVELS + 1] = {nullptr};
  int32_t* next = base + L.sums;
  for (int l = 1; l <= L.levels; ++l) {
    bsum[l] = next;
    boff[l] = next + L.level_n[l];
    next += 2 * L.level_n[l];
  }
  for (int l = 0; l < L.levels; ++l) {
    const dim3 grid((unsigned)L.level_n[l + 1]);
    if (l == 0)
      DVG_LAUNCH(K_GRBM_SUFFSTATS, (distinct_scan_kernel<true, true>), grid, block, 0, s, (const int32_t*)first_ws, T, bsum[1],
                 (const int32_t*)nullptr, (int32_t*)nullptr, (int64_t*)nullptr, (const int32_t*)err);
    else
      DVG_LAUNCH(K_GRBM_SUFFSTATS, (distinct_scan_kernel<false, true>), grid, block, 0, s, (const int32_t*)bsum[l], L.level_n[l],
                 bsum[l + 1], (const int32_t*)nullptr, (int32_t*)nullptr, (int64_t*)nullptr, (const int32_t*)err);
  }
  for (int l = L.levels; l >= 0; --l) {
    const dim3 grid((unsigned)ceil_div(L.level_n[l], DS_TILE));
    const int32_t* off = l == L.levels ? nullptr : boff[l + 1];
    int64_t* total = l == L.levels ? n_distinct : nullptr;
    if (l == 0)
      DVG_LAUNCH(K_GRBM_SUFFSTATS, (distinct_scan_kernel<true, false>), grid, block, 0, s, (const int32_t*)first_ws, T, (int32_t*)nullptr,
                 off, pos, total, (const int32_t*)err);
    else
      DVG_LAUNCH(K_GRBM_SUFFSTATS, (distinct_scan_kernel<false, false>), grid, block, 0, s, (const int32_t*)bsum[l], L.level_n[l],
                 (int32_t*)nullptr, off, boff[l], total, (const int32_t*)err);
  }
  if (id || rep || count || other_hits)
    DVG_LAUNCH(K_GRBM_SUFFSTATS, distinct_emit_kernel, per_row, block, 0, s, (const int32_t*)first_ws, (const int32_t*)pos,
               (const int32_t*)cnt, T, id, rep, count, other_hits, (const int32_t*)err);
  if (other && (other_id || other_hits)) {
    const dim3 grid((unsigned)ceil_div(rows_other << lpr_log2, DS_THREADS));
    if (vec && ds_rows_vec(other, other_row_stride, 1, 0))
      DVG_LAUNCH(K_GRBM_SUFFSTATS, distinct_lookup_kernel<true>, grid, block, 0, s, other, rows_other, other_row_stride, bits, T, rows,
                 row_stride, groups, group_stride, Wi, tail, lpr_log2, hash_mask, (const int32_t*)table, cap_mask, (const int32_t*)pos,
                 other_id, other_hits, (const int32_t*)err);
    else
      DVG_LAUNCH(K_GRBM_SUFFSTATS, distinct_lookup_kernel<false>, grid, block, 0, s, other, rows_other, other_row_stride, bits, T, rows,
                 row_stride, groups, group_stride, Wi, tail, lpr_log2, hash_mask, (const int32_t*)table, cap_mask, (const int32_t*)pos,
                 other_id, other_hits, (const int32_t*)err);
  }
  return DVG_OK;
}
