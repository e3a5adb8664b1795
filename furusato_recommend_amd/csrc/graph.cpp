// Host-side graph build for libmirec.so (runs once per graph) and the
// library's status helpers.
//
// The reference materialises the symmetric edge list [2, 2E] int64
// (model/lgcn.py:53-61) and PyG's gcn_norm recomputes degrees and per-edge
// weights on every LGConv call.  Here the edge list is turned once into a
// destination-major CSR (int64 rowptr, int32 col) by a stable counting sort
// (rows keep the reference's edge order, multi-edges are kept) plus
// dinv = deg^-1/2, which is all the propagation kernel needs.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "mirec.h"

namespace mirec {
thread_local int g_last_hip_error = 0;
}

extern "C" const char *mirec_strerror(int code) {
  switch (code) {
    case MIREC_OK: return "ok";
    case MIREC_ERR_ARG: return "invalid argument";
    case MIREC_ERR_DIM: return "unsupported embedding dim (need 4,8,16,32,64,128 or 256)";
    case MIREC_ERR_HIP: return "HIP runtime error";
    case MIREC_ERR_WORKSPACE: return "workspace too small";
    case MIREC_ERR_RANGE: return "index out of range";
  }
  return "unknown mirec status";
}

extern "C" int mirec_abi_version(void) { return MIREC_ABI_VERSION; }

extern "C" int mirec_last_hip_error(void) { return mirec::g_last_hip_error; }

extern "C" int mirec_struct_sizes(size_t *csr, size_t *prop, size_t *adam_hparams) {
  if (csr == nullptr || prop == nullptr || adam_hparams == nullptr) return MIREC_ERR_ARG;
  *csr = sizeof(mirec_csr_t);
  *prop = sizeof(mirec_prop_t);
  *adam_hparams = sizeof(mirec_adam_hparams_t);
  return MIREC_OK;
}

static void fill_dinv(const int64_t *rowptr, int64_t n, float *dinv) {
  for (int64_t v = 0; v < n; ++v) {
    const int64_t d = rowptr[v + 1] - rowptr[v];
    dinv[v] = d > 0 ? (float)(1.0 / std::sqrt((double)d)) : 0.f;
  }
}

extern "C" int mirec_csr_bipartite(const int64_t *train_user, const int64_t *train_item,
                                   int64_t n_edges, int64_t n_users, int64_t m_items,
                                   int64_t *rowptr, int32_t *col, float *dinv) {
  if (n_edges < 0 || n_users <= 0 || m_items <= 0 || rowptr == nullptr) return MIREC_ERR_ARG;
  if (n_edges > 0 && (train_user == nullptr || train_item == nullptr || col == nullptr))
    return MIREC_ERR_ARG;
  const int64_t n = n_users + m_items;
  if (n >= INT32_MAX) return MIREC_ERR_RANGE;
  std::memset(rowptr, 0, sizeof(int64_t) * (n + 1));
  for (int64_t e = 0; e < n_edges; ++e) {
    const int64_t u = train_user[e], i = train_item[e];
    if (u < 0 || u >= n_users || i < 0 || i >= m_items) return MIREC_ERR_RANGE;
    ++rowptr[u + 1];
    ++rowptr[n_users + i + 1];
  }
  for (int64_t v = 0; v < n; ++v) rowptr[v + 1] += rowptr[v];
  std::vector<int64_t> cur(rowptr, rowptr + n);
  // Destination n_users+i receives from the first half of the reference
  // edge list (user -> item), destination u from the second half
  // (item -> user); both in edge order.
  for (int64_t e = 0; e < n_edges; ++e) {
    const int64_t u = train_user[e], it = n_users + train_item[e];
    col[cur[it]++] = (int32_t)u;
    col[cur[u]++] = (int32_t)it;
  }
  if (dinv != nullptr) fill_dinv(rowptr, n, dinv);
  return MIREC_OK;
}

extern "C" int mirec_csr_from_coo(const int64_t *src, const int64_t *dst, int64_t nnz,
                                  int64_t n_nodes, int64_t *rowptr, int32_t *col, float *dinv) {
  if (nnz < 0 || n_nodes <= 0 || rowptr == nullptr) return MIREC_ERR_ARG;
  if (nnz > 0 && (src == nullptr || dst == nullptr || col == nullptr)) return MIREC_ERR_ARG;
  if (n_nodes >= INT32_MAX) return MIREC_ERR_RANGE;
  std::memset(rowptr, 0, sizeof(int64_t) * (n_nodes + 1));
  for (int64_t e = 0; e < nnz; ++e) {
    if (src[e] < 0 || src[e] >= n_nodes || dst[e] < 0 || dst[e] >= n_nodes)
      return MIREC_ERR_RANGE;
    ++rowptr[dst[e] + 1];
  }
  for (int64_t v = 0; v < n_nodes; ++v) rowptr[v + 1] += rowptr[v];
  std::vector<int64_t> cur(rowptr, rowptr + n_nodes);
  for (int64_t e = 0; e < nnz; ++e) col[cur[dst[e]]++] = (int32_t)src[e];
  if (dinv != nullptr) fill_dinv(rowptr, n_nodes, dinv);
  return MIREC_OK;
}

extern "C" int mirec_csr_entry_order(const int64_t *dst, int64_t nnz, int64_t n_nodes,
                                     int64_t *perm) {
  if (nnz < 0 || n_nodes <= 0) return MIREC_ERR_ARG;
  if (nnz > 0 && (dst == nullptr || perm == nullptr)) return MIREC_ERR_ARG;
  std::vector<int64_t> cur(n_nodes + 1, 0);
  for (int64_t e = 0; e < nnz; ++e) {
    if (dst[e] < 0 || dst[e] >= n_nodes) return MIREC_ERR_RANGE;
    ++cur[dst[e] + 1];
  }
  for (int64_t v = 0; v < n_nodes; ++v) cur[v + 1] += cur[v];
  // the same counting sort as mirec_csr_from_coo, writing the edge's index
  for (int64_t e = 0; e < nnz; ++e) perm[cur[dst[e]]++] = e;
  return MIREC_OK;
}

extern "C" int mirec_csr_long_rows(const int64_t *rowptr, int64_t n_rows, int32_t split,
                                   int64_t *n_long, int64_t *n_seg, int32_t *long_rows,
                                   int64_t *long_segptr, int32_t *seg_row, int64_t *seg_beg) {
  if (rowptr == nullptr || n_rows < 0 || split <= 0 || n_long == nullptr || n_seg == nullptr)
    return MIREC_ERR_ARG;
  const bool fill = long_rows != nullptr;
  if (fill && (long_segptr == nullptr || seg_row == nullptr || seg_beg == nullptr))
    return MIREC_ERR_ARG;
  int64_t nl = 0, ns = 0;
  for (int64_t r = 0; r < n_rows; ++r) {
    const int64_t beg = rowptr[r], deg = rowptr[r + 1] - beg;
    if (deg <= split) continue;
    const int64_t k = (deg + split - 1) / split;
    if (fill) {
      long_rows[nl] = (int32_t)r;
      long_segptr[nl] = ns;
      for (int64_t s = 0; s < k; ++s) {
        seg_row[ns + s] = (int32_t)r;
        seg_beg[ns + s] = beg + s * split;
      }
    }
    ++nl;
    ns += k;
  }
  if (fill) long_segptr[nl] = ns;
  *n_long = nl;
  *n_seg = ns;
  return MIREC_OK;
}

// Rows [0, n_rows) of the CSR with each row's entries sorted ascending (a
// copy: the propagation keeps the reference's edge order).  The samplers test
// "negative item in the user's positives" (negative_sample.py:121-126) by
// binary search in these rows instead of a scan.  Rows are split over up to
// 16 threads by entry count.
extern "C" int mirec_csr_sort_rows(const int64_t *rowptr, const int32_t *col, int64_t n_rows,
                                   int32_t *col_sorted) {
  if (rowptr == nullptr || n_rows < 0 || (rowptr[n_rows] > 0 && (col == nullptr ||
                                                                col_sorted == nullptr)))
    return MIREC_ERR_ARG;
  const int64_t total = rowptr[n_rows] - rowptr[0];
  if (total == 0) return MIREC_OK;
  const int n_thr = (int)std::max<int64_t>(
      1, std::min<int64_t>(16, std::min<int64_t>((int64_t)std::thread::hardware_concurrency(),
                                                 total / (1 << 16) + 1)));
  std::vector<int64_t> cut(n_thr + 1, n_rows);
  cut[0] = 0;
  for (int t = 1; t < n_thr; ++t) {  // first row whose start passes t/n_thr of the entries
    const int64_t want = rowptr[0] + total * t / n_thr;
    cut[t] = std::lower_bound(rowptr, rowptr + n_rows, want) - rowptr;
  }
  auto work = [&](int t) {
    for (int64_t r = cut[t]; r < cut[t + 1]; ++r) {
      const int64_t a = rowptr[r] - rowptr[0], b = rowptr[r + 1] - rowptr[0];
      std::copy(col + rowptr[r], col + rowptr[r + 1], col_sorted + a);
      std::sort(col_sorted + a, col_sorted + b);
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < n_thr; ++t) th.emplace_back(work, t);
  work(0);
  for (auto &x : th) x.join();
  return MIREC_OK;
}

extern "C" size_t mirec_sweep_sizeof(void) { return sizeof(mirec_sweep_t); }

extern "C" int mirec_sweep_shape(int64_t n_rows, int32_t tile_rows, int32_t group_rows,
                                 int32_t *n_tiles, int32_t *groups) {
  if (n_rows < 0 || tile_rows <= 0 || group_rows <= 0 || n_tiles == nullptr || groups == nullptr)
    return MIREC_ERR_ARG;
  const int64_t nt = (n_rows + tile_rows - 1) / tile_rows;
  if (nt >= INT32_MAX) return MIREC_ERR_RANGE;
  *n_tiles = (int32_t)nt;
  *groups = (tile_rows + group_rows - 1) / group_rows;
  return MIREC_OK;
}

// Column-sweep layout (mirec_sweep_t).  Stream (tile, group) covers
// consecutive rows, so its entries occupy the same index range as in the CSR
// (gptr comes straight from rowptr) and the layout is a permutation inside
// each range: sorted by (column, CSR position), i.e. a stable sort by column.
// Tiles are split over up to 16 threads.
extern "C" int mirec_sweep_build(const int64_t *rowptr, const int32_t *col, int64_t row0,
                                 int64_t n_rows, int64_t n_src, int32_t tile_rows,
                                 int32_t group_rows, int64_t *gptr, int32_t *ent) {
  int32_t n_tiles = 0, groups = 0;
  if (rowptr == nullptr || gptr == nullptr || row0 < 0 || n_src < 0) return MIREC_ERR_ARG;
  const int rc = mirec_sweep_shape(n_rows, tile_rows, group_rows, &n_tiles, &groups);
  if (rc != MIREC_OK) return rc;
  const int64_t base = rowptr[row0], total = rowptr[row0 + n_rows] - base;
  if (total < 0 || (total > 0 && (col == nullptr || ent == nullptr))) return MIREC_ERR_ARG;
  auto stream_row = [&](int64_t t, int64_t g) {  // first row (block-relative) of a stream
    const int64_t tile_end = std::min<int64_t>((t + 1) * tile_rows, n_rows);
    return std::min<int64_t>(t * tile_rows + g * group_rows, tile_end);
  };
  for (int64_t t = 0; t < n_tiles; ++t)
    for (int64_t g = 0; g < groups; ++g)
      gptr[t * groups + g] = rowptr[row0 + stream_row(t, g)] - base;
  gptr[(int64_t)n_tiles * groups] = total;
  const int n_thr = (int)std::max<int64_t>(
      1, std::min<int64_t>(16, std::min<int64_t>((int64_t)std::thread::hardware_concurrency(),
                                                 total / (1 << 16) + 1)));
  std::vector<int> bad(n_thr, 0);
  auto work = [&](int th) {
    std::vector<uint64_t> key;
    std::vector<int32_t> lrow;
    for (int64_t t = th; t < n_tiles; t += n_thr) {
      for (int64_t g = 0; g < groups; ++g) {
        const int64_t r0 = stream_row(t, g);
        const int64_t r1 = g + 1 < groups ? stream_row(t, g + 1)
                                          : std::min<int64_t>((t + 1) * tile_rows, n_rows);
        const int64_t e0 = rowptr[row0 + r0], e1 = rowptr[row0 + r1];
        if (e1 - e0 >= INT32_MAX) {
          bad[th] = 1;
          return;
        }
        key.resize(e1 - e0);
        lrow.resize(e1 - e0);
        for (int64_t r = r0; r < r1; ++r)
          for (int64_t e = rowptr[row0 + r]; e < rowptr[row0 + r + 1]; ++e) {
            const int32_t c = col[e];
            if (c < 0 || c >= n_src) {
              bad[th] = 1;
              return;
            }
            key[e - e0] = ((uint64_t)(uint32_t)c << 32) | (uint64_t)(e - e0);
            lrow[e - e0] = (int32_t)(r - t * tile_rows);
          }
        std::sort(key.begin(), key.end());
        int32_t *o = ent + 2 * (e0 - base);
        for (size_t k = 0; k < key.size(); ++k) {
          o[2 * k] = (int32_t)(key[k] >> 32);
          o[2 * k + 1] = lrow[(uint32_t)key[k]];
        }
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < n_thr; ++t) th.emplace_back(work, t);
  work(0);
  for (auto &x : th) x.join();
  for (int b : bad)
    if (b) return MIREC_ERR_RANGE;
  return MIREC_OK;
}

extern "C" size_t mirec_sweep_wave_sizeof(void) { return sizeof(mirec_sweep_wave_t); }

// Per-wave form of the column-sweep layout (mirec_sweep_wave_t).  A wave's
// rows are merged into one stream in (column, CSR position) order and cut
// into steps of 4 slots that name 4 different rows, so the 4 lane groups of
// the wave add into their LDS rows in the same instruction without a race.
// A step takes, among the pending entries less than MIREC_SWEEP_LOOKAHEAD
// merged positions past the oldest pending one, the earliest whose row it
// does not hold yet; an entry skipped for its row keeps every later entry of
// that row out of the step too, so a row's terms keep their merged order.
// What a step cannot fill is padding (local row -1, the column of the slot
// before it); the stream is padded to whole batches the same way.  The padded
// length depends on the data: the streams are scheduled into per-thread
// buffers first, then placed.  Tiles are split over up to 16 threads.
extern "C" int mirec_sweep_wave_build(const int64_t *rowptr, const int32_t *col, int64_t row0,
                                      int64_t n_rows, int64_t src0, int64_t n_src,
                                      int32_t tile_rows, int64_t *wptr, int64_t *slot,
                                      int64_t slot_cap, int64_t *n_slots) {
  constexpr int W = MIREC_SWEEP_WAVES, LOOK = MIREC_SWEEP_LOOKAHEAD, BATCH = MIREC_SWEEP_BATCH;
  if (rowptr == nullptr || wptr == nullptr || n_slots == nullptr || row0 < 0 || src0 < 0 ||
      n_src < 0 || n_rows < 0 || tile_rows <= 0 || slot_cap < 0 ||
      (slot == nullptr && slot_cap > 0))
    return MIREC_ERR_ARG;
  const int64_t n_tiles = (n_rows + tile_rows - 1) / tile_rows;
  if (n_tiles >= INT32_MAX / W) return MIREC_ERR_RANGE;
  const int64_t wave_rows = (tile_rows + W - 1) / W;
  const int64_t total = rowptr[row0 + n_rows] - rowptr[row0];
  if (total < 0 || (total > 0 && col == nullptr)) return MIREC_ERR_ARG;
  const int n_thr = (int)std::max<int64_t>(
      1, std::min<int64_t>(16, std::min<int64_t>((int64_t)std::thread::hardware_concurrency(),
                                                 total / (1 << 16) + 1)));
  std::vector<int> bad(n_thr, 0);
  std::vector<std::vector<int64_t>> buf(n_thr);  // thread th's streams, in its tile order
  auto work = [&](int th) {
    std::vector<uint64_t> key;
    std::vector<int32_t> lrow, mrow, mcol;
    std::vector<char> taken;
    std::vector<int64_t> &o = buf[th];
    for (int64_t t = th; t < n_tiles; t += n_thr) {
      const int64_t tile_end = std::min<int64_t>((t + 1) * tile_rows, n_rows);
      for (int64_t w = 0; w < W; ++w) {
        const int64_t r0 = std::min<int64_t>(t * tile_rows + w * wave_rows, tile_end);
        const int64_t r1 = std::min<int64_t>(r0 + wave_rows, tile_end);
        const int64_t e0 = rowptr[row0 + r0], e1 = rowptr[row0 + r1];
        if (e1 - e0 >= INT32_MAX) {
          bad[th] = 1;
          return;
        }
        const int64_t n = e1 - e0;
        key.resize(n);
        lrow.resize(n);
        for (int64_t r = r0; r < r1; ++r)
          for (int64_t e = rowptr[row0 + r]; e < rowptr[row0 + r + 1]; ++e) {
            const int32_t c = col[e];
            if (c < src0 || c >= src0 + n_src) {
              bad[th] = 1;
              return;
            }
            key[e - e0] = ((uint64_t)(uint32_t)c << 32) | (uint64_t)(e - e0);
            lrow[e - e0] = (int32_t)(r - t * tile_rows);
          }
        std::sort(key.begin(), key.end());
        mrow.resize(n);
        mcol.resize(n);
        for (int64_t k = 0; k < n; ++k) {
          mcol[k] = (int32_t)(key[k] >> 32);
          mrow[k] = lrow[(uint32_t)key[k]];
        }
        taken.assign(n, 0);
        const size_t begin = o.size();
        int64_t head = 0;
        int32_t last_col = 0;
        while (head < n) {
          int32_t rows[4];
          int cnt = 0;
          const int64_t lim = std::min<int64_t>(n, head + LOOK);
          for (int64_t i = head; i < lim && cnt < 4; ++i) {
            if (taken[i]) continue;
            bool clash = false;
            for (int q = 0; q < cnt; ++q) clash |= rows[q] == mrow[i];
            if (clash) continue;
            taken[i] = 1;
            rows[cnt++] = mrow[i];
            last_col = mcol[i];
            o.push_back((int64_t)(((uint64_t)(uint32_t)mrow[i] << 32) | (uint32_t)mcol[i]));
          }
          const int64_t pad = (int64_t)(0xffffffffull << 32 | (uint32_t)last_col);
          for (; cnt < 4; ++cnt) o.push_back(pad);
          while (head < n && taken[head]) ++head;
        }
        const int64_t pad = (int64_t)(0xffffffffull << 32 | (uint32_t)last_col);
        while ((o.size() - begin) % BATCH != 0) o.push_back(pad);
        wptr[t * W + w + 1] = (int64_t)(o.size() - begin);  // length; summed below
      }
    }
  };
  {
    std::vector<std::thread> th;
    for (int t = 1; t < n_thr; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
  }
  for (int b : bad)
    if (b) return MIREC_ERR_RANGE;
  wptr[0] = 0;
  for (int64_t s = 0; s < n_tiles * W; ++s) wptr[s + 1] += wptr[s];
  *n_slots = wptr[n_tiles * W];
  if (*n_slots > slot_cap) return MIREC_ERR_WORKSPACE;
  auto place = [&](int th) {
    const int64_t *src = buf[th].data();
    for (int64_t t = th; t < n_tiles; t += n_thr) {
      const int64_t len = wptr[(t + 1) * W] - wptr[t * W];
      std::copy(src, src + len, slot + wptr[t * W]);
      src += len;
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < n_thr; ++t) th.emplace_back(place, t);
  place(0);
  for (auto &x : th) x.join();
  return MIREC_OK;
}

// The 4-byte form of the slots above: the local row in the top row_bits bits
// (all ones = the padding row -1), the column relative to src0 below them.
extern "C" int mirec_sweep_wave_pack(const int64_t *slot8, int64_t n_slots, int64_t src0,
                                     int64_t n_src, int32_t tile_rows, uint32_t *slot4,
                                     int32_t *row_bits) {
  if (slot8 == nullptr || slot4 == nullptr || row_bits == nullptr || n_slots < 0 || src0 < 0 ||
      n_src < 0 || tile_rows <= 0)
    return MIREC_ERR_ARG;
  int bits = 1;
  while (bits < 31 && ((int64_t)1 << bits) <= (int64_t)tile_rows) ++bits;
  if (((int64_t)1 << bits) <= (int64_t)tile_rows) return MIREC_ERR_RANGE;
  const int col_bits = 32 - bits;
  if (n_src > ((int64_t)1 << col_bits)) return MIREC_ERR_RANGE;
  const uint32_t pad_row = (1u << bits) - 1u;
  const int n_thr = (int)std::max<int64_t>(
      1, std::min<int64_t>(16, std::min<int64_t>((int64_t)std::thread::hardware_concurrency(),
                                                 n_slots / (1 << 20) + 1)));
  std::vector<int> bad(n_thr, 0);
  auto work = [&](int th) {
    const int64_t i0 = n_slots * th / n_thr, i1 = n_slots * (th + 1) / n_thr;
    for (int64_t i = i0; i < i1; ++i) {
      const int64_t c = (int64_t)(uint32_t)((uint64_t)slot8[i] & 0xffffffffull) - src0;
      const int32_t r = (int32_t)(slot8[i] >> 32);
      if (c < 0 || c >= n_src || r < -1 || r >= tile_rows) {
        bad[th] = 1;
        return;
      }
      slot4[i] = ((r < 0 ? pad_row : (uint32_t)r) << col_bits) | (uint32_t)c;
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < n_thr; ++t) th.emplace_back(work, t);
  work(0);
  for (auto &x : th) x.join();
  for (int b : bad)
    if (b) return MIREC_ERR_RANGE;
  *row_bits = bits;
  return MIREC_OK;
}

// Per-user positive CDF for the weighted samplers (the sample_pow option,
// negative_sample.py:53-56): probs[e - rowptr[0]] = the probability of entry
// e of its user row (rows 0 .. n_users - 1, the allPos order), each row's
// probabilities non-negative with a positive sum; cdf[e - rowptr[0]] = the
// inclusive cumulative sum in float64 divided by the row total (numpy's
// choice normalises the same way), kept in float64 — an entry of
// probability 1e-12 after a row mass of 0.5 stays its own CDF step (a float
// CDF would merge it into its neighbour) — the row's last entry exactly 1.
// Empty rows are skipped.
extern "C" int mirec_pos_cdf_build(const int64_t *rowptr, int64_t n_users, const double *probs,
                                   double *cdf) {
  if (rowptr == nullptr || n_users < 0) return MIREC_ERR_ARG;
  const int64_t base = rowptr[0], total = rowptr[n_users] - base;
  if (total > 0 && (probs == nullptr || cdf == nullptr)) return MIREC_ERR_ARG;
  for (int64_t u = 0; u < n_users; ++u) {
    const int64_t a = rowptr[u] - base, b = rowptr[u + 1] - base;
    if (b < a) return MIREC_ERR_ARG;
    if (a == b) continue;
    double s = 0.0;
    for (int64_t e = a; e < b; ++e) {
      if (!(probs[e] >= 0.0) || !std::isfinite(probs[e])) return MIREC_ERR_ARG;
      s += probs[e];
    }
    if (!(s > 0.0)) return MIREC_ERR_ARG;
    double c = 0.0, prev = 0.0;
    for (int64_t e = a; e < b; ++e) {
      c += probs[e];
      double v = c / s;
      v = v < prev ? prev : (v > 1.0 ? 1.0 : v);
      cdf[e] = v;
      prev = v;
    }
    cdf[b - 1] = 1.0;
  }
  return MIREC_OK;
}
