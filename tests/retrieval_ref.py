"""CPU restatement, in float64, of the retrieval rule the GPU kernel implements (rpg_retrieve_cosine_f32): this project's own
statement of the selection step of the reference's obtain_KNNs (dataset_7Scenes_multi.py:238-264), each step citing its lines.
Test helper (like bf16_rounding.py): no test lives here."""
import numpy as np


def cosine_f64(q, db):
    """[G, M] float64 cosine similarities; a zero-norm vector gives 0 (sklearn's normalize leaves a zero row as it is).
    dataset_7Scenes_multi.py:240-242 (``cos_sim(seq_feat, database_feats[idx])`` for every idx, raveled).
    One product-and-sum per (query, row), the same routine for every row: a BLAS matmul picks another code path for the last
    rows of an odd-sized matrix, and bitwise-equal rows would then differ in the last bit by where they sit."""
    q, db = np.asarray(q, dtype=np.float64), np.asarray(db, dtype=np.float64)
    with np.errstate(all="ignore"):
        qn, dn = np.sqrt((q * q).sum(1)), np.sqrt((db * db).sum(1))
        qn[qn == 0] = 1.0
        dn[dn == 0] = 1.0
        qu, du = q / qn[:, None], np.ascontiguousarray(db / dn[:, None])
        return np.stack([(du * qu[g]).sum(1) for g in range(qu.shape[0])]) if qu.shape[0] else np.zeros((0, du.shape[0]))


def allowed_mask(m, q_group, db_group):
    """Row r is allowed unless db_group[r] == q_group; q_group -1 / no groups allow every row.  :245-253: cross_connect is
    groups = index // scene_seq_len, 'drop the query itself' is groups = row index."""
    if db_group is None or q_group is None or int(q_group) == -1:
        return np.ones(m, dtype=bool)
    return np.asarray(db_group) != int(q_group)


def ranking(sims_row, allowed):
    """The allowed rows ordered by (similarity descending, row ascending), a non-finite similarity after every finite one.
    :243 (``np.argsort(1 - dist)``, whose order of exact ties numpy leaves open; here it is defined) and :245-253."""
    s = np.asarray(sims_row, dtype=np.float64)
    rows = np.flatnonzero(allowed)
    fin = np.isfinite(s[rows])
    key = np.where(fin, -s[rows], 0.0) + 0.0          # (-0.0 and +0.0 compare equal anyway)
    order = np.lexsort((rows, key, ~fin))             # last key first: finite before non-finite, then -s, then row
    return rows[order]


def retrieve_ref(q, db, ranks, q_group=None, db_group=None, sims=None):
    """neighbours int64 [G, K]: the rows at positions ranks[g] of each query's ranking (:256-264, the draws being in ranks).
    ``sims``: precomputed [G, M] similarities to rank by instead of the float64 ones (the fp32 CPU reference's, say)."""
    s = cosine_f64(q, db) if sims is None else np.asarray(sims)
    ranks = np.asarray(ranks)
    out = np.empty(ranks.shape, dtype=np.int64)
    for g in range(ranks.shape[0]):
        order = ranking(s[g], allowed_mask(s.shape[1], None if q_group is None else q_group[g], db_group))
        out[g] = order[ranks[g]]
    return out


def n_allowed(m, q_group, db_group):
    if q_group is None or db_group is None:
        return np.full(0 if q_group is None else len(q_group), m, dtype=np.int64)
    return np.asarray([int(allowed_mask(m, g, db_group).sum()) for g in q_group], dtype=np.int64)


def cosine_f32_cpu(q, db):
    """The CPU fp32 reference: sklearn's cosine_similarity on fp32 input (what :240 computes), [G, M] float32."""
    from sklearn.metrics.pairwise import cosine_similarity
    with np.errstate(all="ignore"):
        return cosine_similarity(np.asarray(q, dtype=np.float32), np.asarray(db, dtype=np.float32))
