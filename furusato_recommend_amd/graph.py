"""Device-resident user–item graph (CSR + gcn_norm) for the propagation engine.

Reference: the symmetric edge list of model/lgcn.py:53-61 (users then items
offset by n_users, both directions) and PyG's gcn_norm(add_self_loops=False)
that LGConv recomputes on every call (model/lgcn.py:82; restated in-repo by
model/radj.py:28-36).  Here both are computed once: a destination-major CSR
(int64 rowptr, int32 col, rows in the reference's edge order) and
dinv = deg^-1/2, built on the host by libmirec (mirec_csr_bipartite) and
kept in HBM for the lifetime of the model.

Edge weights (optional): a per-edge float array makes the matrix
A_ij = Σ w over the edges (j → i); the values live beside ``col`` in CSR
order (``val = w[perm]``, ``perm`` = mirec_csr_entry_order) and the degree of
gcn_norm becomes the sum of the weights into a node.  The samplers, the
frontier, GraphSAGE and the data-parallel drivers read the same CSR and use
its structure only: they ignore ``val``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import CSR, Sweep, SweepWave, check, lib

# Rows longer than this are split into segments (load balance on skewed
# item popularity).  2048 neighbours x 256 B = 512 KiB of gather per segment.
DEFAULT_SPLIT = 2048

# Column sweep of the item rows (csrc/prop.hip): the source
# columns are paced in bands of this many bytes of user rows, a workgroup's
# LDS accumulators are capped at SWEEP_LDS_BYTES, and a user block that fits
# one XCD's L2 (4 MiB) gains nothing from the sweep.
SWEEP_BAND_BYTES = 1 << 20
SWEEP_LDS_BYTES = 80 << 10  # the wave form's cap: two workgroups fill a CU's 160 KB
SWEEP_LDS_DEFAULT_BYTES = 64 << 10  # the group form's cap and the item tiles' default cap
SWEEP_L2_BYTES = 4 << 20
SWEEP_WAVES = 8  # MIREC_SWEEP_WAVES: the waves of a sweep workgroup
# The wave form's default tile of the user block: "even" = the
# rule of sweep_user_tile_rows under SWEEP_LDS_BYTES, an int = that many rows.
SWEEP_USER_TILE_ROWS = "even"
# Default of the wave form's slot streams: 4-byte packed slots where the
# block fits them (mirec_sweep_wave_pack), else and when False 8-byte slots.
SWEEP_PACKED = True


def sweep_user_tile_rows(n_rows: int, workgroups: int, cap: int) -> int:
    """Tile of a block swept in passes by ``workgroups`` workgroups.  Every
    pass fetches the whole source block again, so the passes stay as few as
    the cap allows; among the tiles with that many passes, the largest t, a
    whole number of rows per wave, whose ceil(n_rows / t) tiles leave at most
    1 % of the last pass's workgroups without one (passes * workgroups <=
    1.01 * tiles).  The cap if no t does."""
    cap = max(1, int(cap))
    fewest = -(-(-(-n_rows // cap)) // workgroups)
    for t in range(cap - cap % SWEEP_WAVES, 0, -SWEEP_WAVES):
        tiles = -(-n_rows // t)
        passes = -(-tiles // workgroups)
        if tiles < workgroups or passes > fewest:
            break
        if passes * workgroups * 100 <= 101 * tiles:
            return t
    return cap


class SweepLayout:
    """Device arrays of a column-sweep layout and their descriptor."""
    gptr: torch.Tensor
    ent: torch.Tensor
    desc: Sweep

    def ptr(self):
        return ctypes.byref(self.desc)


class SweepWaveLayout:
    """Device arrays of a per-wave column-sweep layout and their descriptor."""
    wptr: torch.Tensor
    slot: torch.Tensor
    desc: SweepWave
    n_entries: int  # real slots (desc.n_slots counts the padding too)

    def ptr(self):
        return ctypes.byref(self.desc)


def _entry_order(dst: np.ndarray, n_nodes: int) -> np.ndarray:
    """perm[k] = index in the edge list of CSR entry k (mirec_csr_from_coo's
    stable order by destination)."""
    dst = np.ascontiguousarray(dst, dtype=np.int64)
    perm = np.empty(dst.shape[0], np.int64)
    check(lib.mirec_csr_entry_order(dst.ctypes.data, dst.shape[0], int(n_nodes),
                                    perm.ctypes.data), "csr_entry_order")
    return perm


def _check_weights(w, n_edges: int, normalize: bool, what: str) -> np.ndarray:
    """Per-edge weights as a contiguous float32 host array (ValueError unless
    one finite entry per edge, non-negative under gcn_norm)."""
    if torch.is_tensor(w):
        w = w.detach().cpu().numpy()
    w = np.asarray(w)
    if w.ndim != 1 or w.shape[0] != n_edges:
        raise ValueError(f"{what}: one weight per edge ({n_edges}), got shape {tuple(w.shape)}")
    w = np.ascontiguousarray(w, dtype=np.float32)
    if not np.isfinite(w).all():
        raise ValueError(f"{what}: weights must be finite")
    if normalize and (w < 0).any():
        raise ValueError(f"{what}: weights must be non-negative with normalize=True "
                         "(deg^-1/2 of a weighted degree)")
    return w


def _weighted_dinv(dst: np.ndarray, w: np.ndarray, n_nodes: int) -> np.ndarray:
    """gcn_norm(add_self_loops=False): deg_i = Σ of the weights into i, in
    float64; dinv = deg^-1/2, 0 where deg == 0."""
    deg = np.bincount(dst, weights=w.astype(np.float64), minlength=n_nodes)
    # 1 / sqrt(deg) rounded to float32 like the unweighted fill: all-ones
    # weights give the unweighted dinv bit for bit
    return np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0).astype(np.float32)


def radj_scales(rowptr, r: float):
    """The two per-node scales of rAdjConv (model/radj.py:28-44),
    y_i = Σ_{(j→i)} x_j / (deg_j^r · deg_i^(1−r)): returns float32 arrays
    ``(a, b)`` with a = deg^−r (the source scale of the forward) and
    b = deg^−(1−r) (its destination scale), deg = the CSR row length
    (multi-edges counted), both 0 where deg = 0, like dinv.  Computed in
    float64 and rounded once.  ValueError unless r is finite and in [0, 1]."""
    r = float(r)
    if not np.isfinite(r) or r < 0.0 or r > 1.0:
        raise ValueError(f"r must be a finite number in [0, 1], got {r!r}")
    rp = np.asarray(rowptr, dtype=np.int64)
    deg = (rp[1:] - rp[:-1]).astype(np.float64)
    pos = deg > 0
    safe = np.where(pos, deg, 1.0)
    a = np.where(pos, safe ** (-r), 0.0).astype(np.float32)
    b = np.where(pos, safe ** (-(1.0 - r)), 0.0).astype(np.float32)
    return a, b


class Graph:
    """CSR of the normalised adjacency Â = D^-1/2 A D^-1/2 (A symmetric)."""

    def __init__(self, rowptr: np.ndarray, col: np.ndarray, dinv: np.ndarray,
                 n_users: int, m_items: int, device, split: int = DEFAULT_SPLIT,
                 symmetric: bool = True, val: np.ndarray | None = None,
                 perm: np.ndarray | None = None, normalize: bool = True):
        self.n_users = int(n_users)
        self.m_items = int(m_items)
        self.n_nodes = int(rowptr.shape[0] - 1)
        self.nnz = int(col.shape[0])
        self.symmetric = symmetric
        self.device = torch.device(device)
        self.rowptr_host = rowptr
        self.col_host = col
        self.dinv_host = dinv
        self.split = int(split)
        n_long, n_seg = ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib.mirec_csr_long_rows(rowptr.ctypes.data, self.n_nodes, self.split,
                                      ctypes.byref(n_long), ctypes.byref(n_seg),
                                      None, None, None, None), "csr_long_rows")
        self.n_long, self.n_seg = n_long.value, n_seg.value
        long_rows = np.zeros(max(self.n_long, 1), np.int32)
        long_segptr = np.zeros(self.n_long + 1, np.int64)
        seg_row = np.zeros(max(self.n_seg, 1), np.int32)
        seg_beg = np.zeros(max(self.n_seg, 1), np.int64)
        if self.n_long:
            check(lib.mirec_csr_long_rows(rowptr.ctypes.data, self.n_nodes, self.split,
                                          ctypes.byref(n_long), ctypes.byref(n_seg),
                                          long_rows.ctypes.data, long_segptr.ctypes.data,
                                          seg_row.ctypes.data, seg_beg.ctypes.data),
                  "csr_long_rows")
        dev = self.device
        self.rowptr = torch.from_numpy(rowptr).to(dev)
        self.col = torch.from_numpy(col if col.size else np.zeros(1, np.int32)).to(dev)
        self.dinv = torch.from_numpy(dinv).to(dev)
        self.long_rows = torch.from_numpy(long_rows).to(dev)
        self.long_segptr = torch.from_numpy(long_segptr).to(dev)
        self.seg_row = torch.from_numpy(seg_row).to(dev)
        self.seg_beg = torch.from_numpy(seg_beg).to(dev)
        self.csr = CSR(rowptr=self.rowptr.data_ptr(), col=self.col.data_ptr(),
                       dinv=self.dinv.data_ptr(), n_rows=self.n_nodes, nnz=self.nnz,
                       split=self.split, _pad=0, n_long=self.n_long, n_seg=self.n_seg,
                       long_rows=self.long_rows.data_ptr(),
                       long_segptr=self.long_segptr.data_ptr(),
                       seg_row=self.seg_row.data_ptr(), seg_beg=self.seg_beg.data_ptr(),
                       col_sorted=None, n_sorted=0, val=None)
        # edge weights: val[k] = w[perm[k]] in CSR order (None = all ones);
        # perm stays on the device for set_edge_weight
        self.normalize = bool(normalize)
        self.val = self.perm = None
        self._coo = None       # host (src, dst) of a from_edge_index graph
        self._w_token = None   # the weight tensor `val` was last refreshed from
        if val is not None:
            self.val = torch.from_numpy(val if val.size else np.zeros(1, np.float32)).to(dev)
            self.perm = torch.from_numpy(perm).to(dev)
            self.csr.val = self.val.data_ptr()
        self.transpose = None  # set for non-symmetric graphs (from_edge_index)
        # r-adjusted normalisation (from_interactions(r != 0.5)): the forward's
        # source scale a = deg^-r and destination scale b = deg^-(1-r) on the
        # device; None = both are dinv and every launch leaves its scale
        # pointers NULL
        self.r = 0.5
        self.scale_src = self.scale_dst = None
        self.col_sorted = None
        self.pos_cdf = None  # weighted positives (set_positive_probs)
        if self.n_users > 0 and self.m_items > 0:
            self._sort_user_rows()

    def _sort_user_rows(self):
        """A sorted copy of the user rows (the positives of every user) for the
        samplers' binary-search membership test (negative_sample.py:121-126)."""
        nu = self.n_users
        n = int(self.rowptr_host[nu] - self.rowptr_host[0])
        cs = np.empty(max(n, 1), np.int32)
        check(lib.mirec_csr_sort_rows(self.rowptr_host.ctypes.data, self.col_host.ctypes.data,
                                      nu, cs.ctypes.data), "csr_sort_rows")
        self.col_sorted = torch.from_numpy(cs).to(self.device)
        self.csr.col_sorted = self.col_sorted.data_ptr()
        self.csr.n_sorted = nu

    # ------------------------------------------------------------------ build
    @classmethod
    def from_interactions(cls, train_user, train_item, n_users: int, m_items: int,
                          device, split: int = DEFAULT_SPLIT, weight=None,
                          r: float = 0.5) -> "Graph":
        """trainUser / trainItem arrays (dataloader.py:93-124) → symmetric CSR.
        ``weight`` (one finite, non-negative value per interaction): both
        directions of interaction e carry weight[e], degrees are weight sums.
        ``r`` (model/radj.py): the normalisation 1 / (deg_j^r · deg_i^(1−r));
        0.5 is this very graph (nothing added), any other value in [0, 1]
        adds the two scale vectors of ``radj_scales`` (``scale_src``,
        ``scale_dst``) and cannot be combined with ``weight``."""
        r = float(r)
        if not np.isfinite(r) or r < 0.0 or r > 1.0:
            raise ValueError(f"r must be a finite number in [0, 1], got {r!r}")
        if r != 0.5 and weight is not None:
            raise ValueError("from_interactions: r != 0.5 cannot be combined with edge weights "
                             "(the scaled kernels carry no values)")
        u = np.ascontiguousarray(np.asarray(train_user, dtype=np.int64))
        i = np.ascontiguousarray(np.asarray(train_item, dtype=np.int64))
        if u.shape != i.shape:
            raise ValueError("train_user and train_item must have the same length")
        n = int(n_users) + int(m_items)
        rowptr = np.empty(n + 1, np.int64)
        col = np.empty(2 * u.shape[0], np.int32)
        dinv = np.empty(n, np.float32)
        check(lib.mirec_csr_bipartite(u.ctypes.data, i.ctypes.data, u.shape[0], int(n_users),
                                      int(m_items), rowptr.ctypes.data, col.ctypes.data,
                                      dinv.ctypes.data), "csr_bipartite")
        if weight is None:
            g = cls(rowptr, col, dinv, n_users, m_items, device, split)
            if r != 0.5:
                a, b = radj_scales(rowptr, r)
                g.r = r
                g.scale_src = torch.from_numpy(a).to(g.device)
                g.scale_dst = torch.from_numpy(b).to(g.device)
            return g
        ne = u.shape[0]
        w = _check_weights(weight, ne, True, "from_interactions")
        # the CSR is the stable destination sort of the reference's doubled
        # edge list (user -> item, then item -> user); edge e of it is
        # interaction e mod ne
        dst2 = np.concatenate([i + int(n_users), u])
        perm = _entry_order(dst2, n) % max(ne, 1)
        dinv = _weighted_dinv(dst2, np.concatenate([w, w]), n)
        return cls(rowptr, col, dinv, n_users, m_items, device, split, val=w[perm], perm=perm)

    @classmethod
    def from_edge_index(cls, edge_index, n_nodes: int, device,
                        split: int = DEFAULT_SPLIT, normalize: bool = True,
                        edge_weight=None) -> "Graph":
        """Generic LGConv graph: edge_index[0] = source, [1] = target (PyG
        flow source_to_target; degree = in-degree at the target, multi-edges
        counted).  ``normalize=False``: plain neighbour sum (dinv = 1).
        ``edge_weight`` (one finite value per edge, non-negative with
        ``normalize``): A_ij = Σ of the weights of the edges (j → i), each
        duplicate edge its own entry; degree = Σ of the weights into the
        target (PyG gcn_norm, add_self_loops=False)."""
        ei = np.ascontiguousarray(np.asarray(edge_index, dtype=np.int64))
        src, dst = np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1])
        nnz = src.shape[0]
        w = None if edge_weight is None else _check_weights(edge_weight, nnz, normalize,
                                                            "from_edge_index")
        rowptr = np.empty(n_nodes + 1, np.int64)
        col = np.empty(nnz, np.int32)
        dinv = np.empty(n_nodes, np.float32)
        check(lib.mirec_csr_from_coo(src.ctypes.data, dst.ctypes.data, nnz, n_nodes,
                                     rowptr.ctypes.data, col.ctypes.data, dinv.ctypes.data),
              "csr_from_coo")
        if not normalize:
            dinv[:] = 1.0
        elif w is not None:
            dinv = _weighted_dinv(dst, w, n_nodes)
        # Is the edge multiset symmetric?  Then Âᵀ = Â (same CSR for backward).
        # With weights: the multiset of (src, dst, weight) triples.
        kf, kb = src * n_nodes + dst, dst * n_nodes + src
        if w is None:
            symmetric = bool(np.array_equal(np.sort(kf), np.sort(kb)))
            g = cls(rowptr, col, dinv, n_nodes, 0, device, split, symmetric=symmetric,
                    normalize=normalize)
        else:
            of, ob = np.lexsort((w, kf)), np.lexsort((w, kb))
            symmetric = bool(np.array_equal(kf[of], kb[ob]) and np.array_equal(w[of], w[ob]))
            perm = _entry_order(dst, n_nodes)
            g = cls(rowptr, col, dinv, n_nodes, 0, device, split, symmetric=symmetric,
                    val=w[perm], perm=perm, normalize=normalize)
        g._coo = (src, dst)
        if not symmetric:
            g._build_transpose(w)
        return g

    def _build_transpose(self, w: np.ndarray | None):
        """Backward of y = Â x is x̄ = Âᵀ ȳ: CSR by source, same dinv, the
        values permuted into its own entry order."""
        src, dst = self._coo
        n_nodes, nnz = self.n_nodes, src.shape[0]
        rowptr_t = np.empty(n_nodes + 1, np.int64)
        col_t = np.empty(nnz, np.int32)
        check(lib.mirec_csr_from_coo(dst.ctypes.data, src.ctypes.data, nnz, n_nodes,
                                     rowptr_t.ctypes.data, col_t.ctypes.data, None),
              "csr_from_coo(transpose)")
        kw = {}
        if w is not None:
            perm_t = _entry_order(src, n_nodes)
            kw = dict(val=w[perm_t], perm=perm_t)
        self.transpose = Graph(rowptr_t, col_t, self.dinv_host, n_nodes, 0, self.device,
                               self.split, normalize=self.normalize, **kw)

    def set_edge_weight(self, w: torch.Tensor) -> None:
        """Refresh the values of a weighted ``normalize=False`` graph from a
        device tensor of per-edge weights (edge order of the build): one
        gather through ``perm`` on the current stream, no host sync and no
        rebuild (dinv = 1 does not depend on the weights).  Nothing here can
        look at the new values, so a from_edge_index graph that was symmetric
        for its first weights gets its transpose now (once, host work on the
        structure only) and is treated as non-symmetric from then on."""
        if self.val is None:
            raise ValueError("set_edge_weight: the graph was built without edge weights")
        if self.normalize:
            raise ValueError("set_edge_weight: dinv of a normalize=True graph depends on the "
                             "weights; rebuild the graph instead")
        n_edges = self.nnz // 2 if self._coo is None else self.nnz
        if w.dim() != 1 or w.shape[0] != n_edges:
            raise ValueError(f"set_edge_weight: one weight per edge ({n_edges}), "
                             f"got shape {tuple(w.shape)}")
        w = w.detach().to(device=self.device, dtype=torch.float32)
        if self.nnz:
            torch.index_select(w, 0, self.perm, out=self.val[: self.nnz])
        if self._coo is not None:
            if self.transpose is None:
                self._build_transpose(np.zeros(self.nnz, np.float32))
                self.symmetric = False
            t = self.transpose
            if self.nnz:
                torch.index_select(w, 0, t.perm, out=t.val[: self.nnz])
        self._w_token = None

    # ------------------------------------------------------------ column sweep
    def sweep_layout(self, dim: int, tile_rows: int | None = None,
                     group_rows: int | None = None, band_rows: int | None = None):
        """The column-ordered layout of the item rows (mirec_sweep_t) for
        width ``dim``, or None when the graph does not qualify: edge weights, not a
        bipartite user–item graph, a long row anywhere (n_seg > 0), no sweep
        kernel for the width; and, with the default sizes, fewer item rows
        than CUs or a user block that fits one XCD's L2.  Defaults: two tiles
        per CU (all resident at once), half as many lane groups as the kernel has,
        bands of SWEEP_BAND_BYTES of user rows.  Explicit sizes (tests, tuning)
        skip the two size conditions.  Built once per (graph, sizes)."""
        key = ("sweep", dim, tile_rows, group_rows, band_rows)
        cache = self.__dict__.setdefault("_sweeps", {})
        if key in cache:
            return cache[key]
        cache[key] = lay = self._build_sweep(dim, tile_rows, group_rows, band_rows)
        return lay

    def _build_sweep(self, dim, tile_rows, group_rows, band_rows):
        nu, mi = self.n_users, self.m_items
        if self.val is not None:  # the sweep layout carries no values
            return None
        max_groups = int(lib.mirec_sweep_groups(dim))
        if not (self.symmetric and nu > 0 and mi > 0 and nu + mi == self.n_nodes):
            return None
        if self.n_seg > 0 or max_groups == 0 or self.device.type != "cuda":
            return None
        explicit = not (tile_rows is None and group_rows is None and band_rows is None)
        row_bytes = dim * 4
        max_tile = SWEEP_LDS_DEFAULT_BYTES // row_bytes
        if not explicit:
            n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count
            if mi < n_cu or nu * row_bytes <= SWEEP_L2_BYTES:
                return None
        if tile_rows is None:
            n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count
            tile_rows = min(max_tile, max(1, -(-mi // (2 * n_cu))))
        if group_rows is None:
            # half the workgroup's lane groups, each with twice the rows: 1.315
            # against 1.353 ms per full C2 launch
            group_rows = -(-tile_rows // max(1, max_groups // 2))
        if band_rows is None:
            band_rows = max(1, SWEEP_BAND_BYTES // row_bytes)
        tile_rows, group_rows, band_rows = int(tile_rows), int(group_rows), int(band_rows)
        n_tiles, groups = ctypes.c_int32(0), ctypes.c_int32(0)
        check(lib.mirec_sweep_shape(mi, tile_rows, group_rows, ctypes.byref(n_tiles),
                                    ctypes.byref(groups)), "sweep_shape")
        if tile_rows > max_tile or groups.value > max_groups or band_rows <= 0:
            raise ValueError(f"sweep sizes out of range: tile_rows {tile_rows} (max {max_tile}), "
                             f"{groups.value} groups (max {max_groups}), band_rows {band_rows}")
        n_ent = int(self.rowptr_host[nu + mi] - self.rowptr_host[nu])
        gptr = np.empty(n_tiles.value * groups.value + 1, np.int64)
        ent = np.zeros(2 * max(n_ent, 1), np.int32)
        check(lib.mirec_sweep_build(self.rowptr_host.ctypes.data, self.col_host.ctypes.data, nu,
                                    mi, nu, tile_rows, group_rows, gptr.ctypes.data,
                                    ent.ctypes.data), "sweep_build")
        lay = SweepLayout()
        lay.gptr = torch.from_numpy(gptr).to(self.device)
        lay.ent = torch.from_numpy(ent).to(self.device)
        lay.desc = Sweep(row0=nu, n_rows=mi, n_src=nu, tile_rows=tile_rows,
                         group_rows=group_rows, groups=groups.value, n_tiles=n_tiles.value,
                         band_rows=band_rows, _pad=0, gptr=lay.gptr.data_ptr(),
                         ent=lay.ent.data_ptr())
        return lay

    def sweep_wave_layout(self, dim: int, block: str = "items", tile_rows: int | None = None,
                          band_rows: int | None = None, max_grid: int | None = None,
                          packed: bool | None = None):
        """The per-wave form of the column-sweep layout (mirec_sweep_wave_t,
        DESIGN.md §14) of the item rows (``block="items"``, gathering from the
        user block) or of the user rows (``"users"``, gathering from the item
        block), or None when the graph does not qualify: the conditions of
        ``sweep_layout``, and for the user rows with default sizes an item
        block larger than one XCD's L2.  Defaults: for the items two tiles per
        CU (one pass), for the users tiles of SWEEP_USER_TILE_ROWS swept in
        passes by two workgroups per CU; bands of SWEEP_BAND_BYTES of source rows.
        ``max_grid`` caps the workgroups launched (tests force several passes
        on a small graph).  ``packed`` (None: SWEEP_PACKED) uploads the slots
        in their 4-byte form when the block fits it (``desc.row_bits`` > 0),
        the 8-byte slots otherwise.  Built once per (graph, sizes, form)."""
        packed = SWEEP_PACKED if packed is None else bool(packed)
        key = ("wave", dim, block, tile_rows, band_rows, max_grid, packed)
        cache = self.__dict__.setdefault("_sweeps", {})
        if key in cache:
            return cache[key]
        cache[key] = lay = self._build_sweep_wave(dim, block, tile_rows, band_rows, max_grid,
                                                  packed)
        return lay

    def _build_sweep_wave(self, dim, block, tile_rows, band_rows, max_grid, packed):
        nu, mi = self.n_users, self.m_items
        if block not in ("items", "users"):
            raise ValueError(f"block: 'items' or 'users', got {block!r}")
        if self.val is not None:  # the sweep layouts carry no values
            return None
        if not (self.symmetric and nu > 0 and mi > 0 and nu + mi == self.n_nodes):
            return None
        if self.n_seg > 0 or lib.mirec_sweep_groups(dim) == 0 or self.device.type != "cuda":
            return None
        explicit = not (tile_rows is None and band_rows is None)
        row_bytes = dim * 4
        max_tile = SWEEP_LDS_BYTES // row_bytes
        n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count
        if not explicit:
            if mi < n_cu or nu * row_bytes <= SWEEP_L2_BYTES:
                return None
            if block == "users" and mi * row_bytes <= SWEEP_L2_BYTES:
                return None
        row0, n_rows, src0, n_src = (nu, mi, 0, nu) if block == "items" else (0, nu, nu, mi)
        if tile_rows is None:
            if block == "items":
                tile_rows = min(SWEEP_LDS_DEFAULT_BYTES // row_bytes,
                                max(1, -(-mi // (2 * n_cu))))
            elif SWEEP_USER_TILE_ROWS == "even":
                tile_rows = sweep_user_tile_rows(nu, 2 * n_cu, max_tile)
            else:
                tile_rows = int(SWEEP_USER_TILE_ROWS)
        if band_rows is None:
            band_rows = max(1, SWEEP_BAND_BYTES // row_bytes)
        tile_rows, band_rows = int(tile_rows), int(band_rows)
        if not 0 < tile_rows <= max_tile or band_rows <= 0:
            raise ValueError(f"sweep sizes out of range: tile_rows {tile_rows} (max {max_tile}), "
                             f"band_rows {band_rows}")
        n_tiles = -(-n_rows // tile_rows)
        n_ent = int(self.rowptr_host[row0 + n_rows] - self.rowptr_host[row0])
        if n_ent == 0:
            return None
        wptr = np.empty(n_tiles * SWEEP_WAVES + 1, np.int64)
        # room for the usual padding; the builder says what it needs otherwise
        slot = np.empty(n_ent + n_ent // 8 + 16 * n_tiles * SWEEP_WAVES, np.int64)
        n_slots = ctypes.c_int64(0)
        for _ in range(2):
            rc = lib.mirec_sweep_wave_build(self.rowptr_host.ctypes.data,
                                            self.col_host.ctypes.data, row0, n_rows, src0, n_src,
                                            tile_rows, wptr.ctypes.data, slot.ctypes.data,
                                            slot.shape[0], ctypes.byref(n_slots))
            if rc != _lib.ERR_WORKSPACE:
                break
            slot = np.empty(n_slots.value, np.int64)
        check(rc, "sweep_wave_build")
        grid = min(n_tiles, 2 * n_cu)
        if max_grid is not None:
            grid = max(1, min(grid, int(max_grid)))
        lay = SweepWaveLayout()
        lay.n_entries = n_ent
        lay.wptr = torch.from_numpy(wptr).to(self.device)
        slot, row_bits = slot[:n_slots.value], ctypes.c_int32(0)
        if packed:
            slot4 = np.empty(n_slots.value, np.uint32)
            rc = lib.mirec_sweep_wave_pack(slot.ctypes.data, n_slots.value, src0, n_src,
                                           tile_rows, slot4.ctypes.data, ctypes.byref(row_bits))
            if rc == _lib.ERR_RANGE:  # the block does not fit 32 bits: 8-byte slots
                row_bits.value = 0
            else:
                check(rc, "sweep_wave_pack")
                slot = slot4.view(np.int32)
        lay.slot = torch.from_numpy(slot).to(self.device)
        lay.desc = SweepWave(row0=row0, n_rows=n_rows, src0=src0, n_src=n_src,
                             n_slots=n_slots.value, tile_rows=tile_rows,
                             wave_rows=-(-tile_rows // SWEEP_WAVES), n_tiles=n_tiles,
                             band_rows=band_rows, grid=grid, row_bits=row_bits.value,
                             wptr=lay.wptr.data_ptr(), slot=lay.slot.data_ptr())
        return lay

    def set_positive_probs(self, probs) -> None:
        """Per-user positive probabilities for the samplers (the sample_pow
        option of negative_sample.py:22-56: ``probs[u]`` is the probability
        vector over ``allPos[u]``, which is this CSR's user-row order).
        ``probs``: a sequence of per-user arrays, or one flat float array of
        the user rows' entries; ``None`` restores the uniform positive.  The
        row CDFs are built on the host (mirec_pos_cdf_build) and kept in HBM;
        every sampler call on this graph then draws its positive from them."""
        if probs is None:
            self.pos_cdf = None
            return
        nu = self.n_users
        n = int(self.rowptr_host[nu] - self.rowptr_host[0])
        if isinstance(probs, np.ndarray) and probs.ndim == 1:
            flat = np.ascontiguousarray(probs, dtype=np.float64)
        else:
            if len(probs) != nu:
                raise ValueError(f"probs: one array per user ({nu}), got {len(probs)}")
            deg = np.diff(self.rowptr_host[: nu + 1])
            parts = [np.asarray(p, dtype=np.float64).reshape(-1) for p in probs]
            bad = [u for u, (p, d) in enumerate(zip(parts, deg)) if p.size != d]
            if bad:
                raise ValueError(f"probs[{bad[0]}] has {parts[bad[0]].size} entries, "
                                 f"the user has {deg[bad[0]]} positives")
            flat = np.concatenate(parts) if parts else np.zeros(0)
        if flat.size != n:
            raise ValueError(f"probs: {flat.size} entries for {n} user-row entries")
        cdf = np.empty(max(n, 1), np.float64)
        check(lib.mirec_pos_cdf_build(self.rowptr_host.ctypes.data, nu, flat.ctypes.data,
                                      cdf.ctypes.data), "pos_cdf_build")
        self.pos_cdf = torch.from_numpy(cdf).to(self.device)

    # ---------------------------------------------------------------- helpers
    def degree(self) -> np.ndarray:
        return np.diff(self.rowptr_host)

    def csr_ptr(self):
        return ctypes.byref(self.csr)

    def partial_buffer(self, dim: int) -> torch.Tensor | None:
        if self.n_seg == 0:
            return None
        key = ("partial", dim)
        buf = getattr(self, "_bufs", {}).get(key)
        if buf is None:
            buf = torch.empty(self.n_seg, dim, dtype=torch.float32, device=self.device)
            self._bufs = getattr(self, "_bufs", {})
            self._bufs[key] = buf
        return buf

    def bytes_per_layer(self, dim: int, fused_acc: bool = True) -> int:
        """Algorithmic HBM bytes of one propagation layer."""
        n, nnz = self.n_nodes, self.nnz
        b = nnz * dim * 4 + nnz * 4 + (n + 1) * 8 + n * 4 + n * dim * 4
        if self.val is not None:
            b += nnz * 4  # the per-entry weight
        if fused_acc:
            b += 2 * n * dim * 4
        return b


def positive_probs(config: dict):
    """The per-user positive probabilities a model config asks for: the
    reference's ``sample_pow`` (parse.py:48; negative_sample.py:22-38 loads
    ``data/sample_prob/sample_prob_<pow>.pkl``, a list of per-user arrays over
    allPos[u]) comes here as ``config["sample_probs"]`` — the arrays
    themselves (this package does not unpickle files).  None = uniform."""
    probs = config.get("sample_probs")
    if probs is None and float(config.get("sample_pow", 0) or 0) != 0:
        raise ValueError("sample_pow != 0: pass the per-user probabilities as "
                         "config['sample_probs'] (the arrays of sample_prob_*.pkl)")
    return probs


_ = _lib  # keep the module import explicit for readers
