"""float64 restatements for the full-rank evaluation tests:
brute-force rank counts, the derived error bracket of a count, and the
metrics computed directly from full score rows."""
import numpy as np


def pair_slots(tptr):
    tptr = np.asarray(tptr, dtype=np.int64)
    return np.repeat(np.arange(len(tptr) - 1), np.diff(tptr))


def make_targets(lists):
    """Per-slot item lists -> (tptr, targets)."""
    tptr = np.zeros(len(lists) + 1, dtype=np.int64)
    tptr[1:] = np.cumsum([len(x) for x in lists])
    flat = [np.asarray(x, dtype=np.int64) for x in lists if len(x)]
    return tptr, (np.concatenate(flat) if flat else np.zeros(0, dtype=np.int64))


def train_mask(train_lists, users, m_items):
    """bool [len(users), m_items]: item is a train positive of users[r]
    (train_lists = None: nothing is)."""
    mask = np.zeros((len(users), m_items), dtype=bool)
    if train_lists is not None:
        for r, u in enumerate(np.asarray(users).tolist()):
            mask[r, np.asarray(train_lists[u], dtype=np.int64)] = True
    return mask


def brute_counts(s, train, tptr, targets):
    """score / gt / eq / eq_lower / masked of every pair from the score rows
    s [n, M] (float64) and the train mask [n, M], by the definition."""
    slot = pair_slots(tptr)
    nt = len(targets)
    ids = np.arange(s.shape[1])
    score = np.zeros(nt)
    gt, eq, eql = (np.zeros(nt, dtype=np.int64) for _ in range(3))
    masked = np.zeros(nt, dtype=bool)
    for p in range(nt):
        r, t = slot[p], targets[p]
        live = ~train[r]
        score[p] = s[r, t]
        masked[p] = train[r, t]
        gt[p] = np.sum(live & (s[r] > s[r, t]))
        tie = live & (s[r] == s[r, t])
        eq[p] = np.sum(tie)
        eql[p] = np.sum(tie & (ids < t))
    return score, gt, eq, eql, masked


def gamma(d):
    """γ_d of the f32 dot-product bound |fl(u·i) - u·i| <= γ_d Σ|u_k||i_k|,
    any summation order, fused or not (u = 2^-24)."""
    u = 2.0 ** -24
    return d * u / (1.0 - d * u)


def bracket(U, I, train, tptr, targets):
    """(lower, upper) per pair: with s the float64 scores over J \\ {t} and
    e_j = γ_d Σ_k |u_k||i_jk|, lower = #{s_j - s_t > e_j + e_t} items are
    above t whatever the f32 rounding did, upper = #{s_j - s_t >= -(e_j +
    e_t)} can be above or tied.  So lower <= gt and gt + eq - 1 <= upper."""
    U, I = np.asarray(U, dtype=np.float64), np.asarray(I, dtype=np.float64)
    s = U @ I.T
    e = gamma(U.shape[1]) * (np.abs(U) @ np.abs(I).T)
    slot = pair_slots(tptr)
    lower, upper = (np.zeros(len(targets), dtype=np.int64) for _ in range(2))
    for p in range(len(targets)):
        r, t = slot[p], targets[p]
        live = ~train[r]
        live[t] = False
        diff, tol = s[r] - s[r, t], e[r] + e[r, t]
        lower[p] = np.sum(live & (diff > tol))
        upper[p] = np.sum(live & (diff >= -tol))
    return lower, upper


def sorted_lists(s, train):
    """Every user's non-train items in score_topk's order (score descending,
    ties to the lower id), padded with -1 to M columns."""
    n, m = s.shape
    out = np.full((n, m), -1, dtype=np.int64)
    ids = np.arange(m)
    for r in range(n):
        order = np.lexsort((ids, -s[r]))
        order = order[~train[r, order]]
        out[r, :len(order)] = order
    return out


def brute_mrr_auc(s, train, test_lists):
    """(Σ_u 1 / best rank, Σ_u AUC_u, users in the AUC sum) straight from the
    rows: rank by position in the sorted non-train list; AUC_u the
    Mann-Whitney statistic of the unmasked test items against the non-train,
    non-test items, ties at ½."""
    lists = sorted_lists(s, train)
    mrr, auc, n_auc = 0.0, 0.0, 0
    for r, items in enumerate(test_lists):
        pos = [t for t in sorted(set(items)) if not train[r, t]]
        if not pos:
            continue
        mrr += 1.0 / min(int(np.nonzero(lists[r] == t)[0][0]) + 1 for t in pos)
        neg = ~train[r]
        neg[pos] = False
        sn = s[r, neg]
        if sn.size == 0:
            continue
        wins = sum(np.sum(s[r, t] > sn) + 0.5 * np.sum(s[r, t] == sn) for t in pos)
        auc += wins / (len(pos) * sn.size)
        n_auc += 1
    return mrr, auc, n_auc
