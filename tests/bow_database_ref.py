"""data::bow_database (src/PLPSLAM/data/bow_database.cc:97-378) and loop_detector::compute_min_score_in_covisibilities
(module/loop_detector.cc:238-266) restated literally in Python: key-frame objects, an inverted index word -> list of key frames, dicts and sets,
the four helper functions as the reference writes them, and an np.float32 / np.float64 scalar for every arithmetic step.  It shares nothing with
the kernels' formulation (rows, masks, bitmaps).  The score is DBoW2's L1Scoring::score restated from the published algorithm (DBoW2 is not in the
reference tree: parity unpinned), with its lower_bound jumps.

Also the scene builder of the bow_database tests: word sets made directly, no descriptors -- "places" of key frames that share a planted core
of a query's words, with normalised random values -- and the census of the branches a scene reaches."""
import bisect

import numpy as np

f32, f64 = np.float32, np.float64


class KeyFrame:
    def __init__(self, id_, bow_vec):
        self.id_ = id_
        self.bow_vec_ = bow_vec            # std::map<WordId, WordValue>: a dict in ascending key order
        self.top_covisibilities = []       # graph_node_->get_top_n_covisibilities(10)
        self.erased = False                # will_be_erased()

    def will_be_erased(self):
        return self.erased


def l1_score(v1, v2):
    """DBoW2 L1Scoring::score(v1, v2): two iterators, lower_bound jumps, one double accumulator"""
    k1, k2 = list(v1.keys()), list(v2.keys())
    i, j = 0, 0
    score = f64(0.0)
    while i < len(k1) and j < len(k2):
        if k1[i] == k2[j]:
            vi, wi = f64(v1[k1[i]]), f64(v2[k2[j]])
            score = f64(score + f64(f64(f64(np.fabs(f64(vi - wi))) - f64(np.fabs(vi))) - f64(np.fabs(wi))))
            i += 1
            j += 1
        elif k1[i] < k2[j]:
            i = bisect.bisect_left(k1, k2[j])      # v1_it = v1.lower_bound(v2_it->first)
        else:
            j = bisect.bisect_left(k2, k1[i])
    return f64(f64(-score) / f64(2.0))


class BowDatabase:
    def __init__(self):
        self.keyfrms_in_node_ = {}
        self.initialize()

    def add_keyframe(self, keyfrm):
        for word in keyfrm.bow_vec_:
            self.keyfrms_in_node_.setdefault(word, []).append(keyfrm)

    def erase_keyframe(self, keyfrm):
        for word in keyfrm.bow_vec_:
            lst = self.keyfrms_in_node_.get(word)
            if lst is None:
                continue
            for n, kf in enumerate(lst):
                if kf is keyfrm:
                    del lst[n]
                    break

    def initialize(self):
        self.init_candidates_ = set()
        self.num_common_words_ = {}
        self.scores_ = {}
        self.score_keyfrm_pairs_ = []
        self.total_score_keyfrm_pairs_ = []

    def set_candidates_sharing_words(self, qry_bow_vec, keyfrms_to_reject=frozenset()):
        self.init_candidates_ = set()
        self.num_common_words_ = {}
        for word in qry_bow_vec:
            if word not in self.keyfrms_in_node_:
                continue
            for kf in self.keyfrms_in_node_[word]:
                if kf not in self.num_common_words_:
                    self.num_common_words_[kf] = 0
                    if kf not in keyfrms_to_reject:
                        self.init_candidates_.add(kf)
                self.num_common_words_[kf] += 1
        return len(self.init_candidates_) != 0

    def compute_scores(self, qry_bow_vec, min_num_common_words_thr):
        self.scores_ = {}
        for candidate in self.init_candidates_:
            if min_num_common_words_thr < self.num_common_words_[candidate]:
                self.scores_[candidate] = f32(l1_score(qry_bow_vec, candidate.bow_vec_))     # const float score = bow_vocab_->score(...)
        return len(self.scores_) != 0

    def align_scores_and_keyframes(self, min_num_common_words_thr, min_score):
        self.score_keyfrm_pairs_ = []
        for candidate in self.init_candidates_:
            if min_num_common_words_thr < self.num_common_words_[candidate]:
                score = self.scores_[candidate]
                if min_score <= score:
                    self.score_keyfrm_pairs_.append((score, candidate))
        return len(self.score_keyfrm_pairs_) != 0

    def align_total_scores_and_keyframes(self, min_num_common_words_thr, min_score):
        self.total_score_keyfrm_pairs_ = []
        self.total_owner_ = []                     # not in the reference: which key frame a pair was made for, to lay the results out by row
        best_total_score = f32(min_score)
        for score, keyfrm in self.score_keyfrm_pairs_:
            total_score = f32(score)
            best_score = f32(score)
            best_keyframe = keyfrm
            for covisibility in keyfrm.top_covisibilities:
                if covisibility in self.init_candidates_ and min_num_common_words_thr < self.num_common_words_[covisibility]:
                    total_score = f32(total_score + self.scores_[covisibility])
                    if best_score < self.scores_[covisibility]:
                        best_score = self.scores_[covisibility]
                        best_keyframe = covisibility
            self.total_score_keyfrm_pairs_.append((total_score, best_keyframe))
            self.total_owner_.append(keyfrm)
            if best_total_score < total_score:
                best_total_score = total_score
        return best_total_score

    def acquire_candidates(self, qry_bow_vec, keyfrms_to_reject, min_score):
        """acquire_loop_candidates (:97-168); acquire_relocalization_candidates (:170-236) is the same with no rejected key frames and
        min_score 0.0.  Returns (final_candidates set, status, max_num_common_words, best_total_score): status 1 / 2 / 3 = the early return
        of :111 / :134 / :140, where best_total_score is reported as min_score (the reference has not computed one)."""
        min_score = f32(min_score)
        self.initialize()
        if not self.set_candidates_sharing_words(qry_bow_vec, keyfrms_to_reject):
            return set(), 1, 0, min_score
        max_num_common_words = 0
        for candidate in self.init_candidates_:
            if max_num_common_words < self.num_common_words_[candidate]:
                max_num_common_words = self.num_common_words_[candidate]
        min_num_common_words = int(f32(f32(0.8) * f32(max_num_common_words)))      # static_cast<unsigned int>(0.8f * max_num_common_words)
        self.min_num_common_words = min_num_common_words
        if not self.compute_scores(qry_bow_vec, min_num_common_words):
            return set(), 2, max_num_common_words, min_score
        if not self.align_scores_and_keyframes(min_num_common_words, min_score):
            return set(), 3, max_num_common_words, min_score
        best_total_score = self.align_total_scores_and_keyframes(min_num_common_words, min_score)
        min_total_score = f32(f32(0.75) * best_total_score)
        final_candidates = set()
        for total_score, keyfrm in self.total_score_keyfrm_pairs_:
            if min_total_score < total_score:
                final_candidates.add(keyfrm)
        return final_candidates, 0, max_num_common_words, best_total_score


def compute_min_score_in_covisibilities(keyfrm, covisibilities):
    """loop_detector.cc:238-266 (USE_DBOW2)"""
    min_score = f32(1.0)
    for covisibility in covisibilities:
        if covisibility.will_be_erased():
            continue
        score = f32(l1_score(keyfrm.bow_vec_, covisibility.bow_vec_))
        if score < min_score:
            min_score = score
    return min_score


# ---- from arrays to the restatement and back
def bow_vec_of(word, value, n):
    return {int(w): f64(v) for w, v in zip(word[:n], value[:n])}


def run(scene, use_reject=True, use_min_score=True):
    """the restatement on a scene (the arrays of scene()): every output of plp_bow_query_* as arrays [Q][N] / [Q]"""
    N, Q = len(scene["db_n"]), len(scene["q_n"])
    kfs = [KeyFrame(k, bow_vec_of(scene["db_word"][k], scene["db_value"][k], scene["db_n"][k])) for k in range(N)]
    db = BowDatabase()
    for k in range(N):
        if scene["db_alive"][k]:
            db.add_keyframe(kfs[k])
    for k in range(N):
        kfs[k].top_covisibilities = [kfs[c] for c in scene["covis"][k][:scene["n_covis"][k]]]
    out = dict(common=np.zeros((Q, N), np.uint32), score=np.full((Q, N), -1, np.float32), total=np.full((Q, N), -1, np.float32),
               best_kf=np.full((Q, N), -1, np.int32), final=np.zeros((Q, N), np.uint8), n_final=np.zeros(Q, np.int32),
               max_common=np.zeros(Q, np.uint32), best_total=np.zeros(Q, np.float32), status=np.zeros(Q, np.uint8))
    for q in range(Q):
        qv = bow_vec_of(scene["q_word"][q], scene["q_value"][q], scene["q_n"][q])
        reject = {kfs[k] for k in range(N) if use_reject and scene["reject"][q][k]}
        ms = scene["min_score"][q] if use_min_score else f32(0.0)
        final, status, mx, best_total = db.acquire_candidates(qv, reject, ms)
        for kf, c in db.num_common_words_.items():
            out["common"][q, kf.id_] = c
        for kf, s in db.scores_.items():
            out["score"][q, kf.id_] = s
        if status == 0:
            for (tot, best), kf in zip(db.total_score_keyfrm_pairs_, db.total_owner_):
                out["total"][q, kf.id_] = tot
                out["best_kf"][q, kf.id_] = best.id_
        for kf in final:
            out["final"][q, kf.id_] = 1
        out["n_final"][q], out["max_common"][q], out["best_total"][q], out["status"][q] = len(final), mx, best_total, status
    return out


# ---- scenes
def normalised(rng, n):
    v = rng.random(n) + 0.05
    return v / v.sum()


def planted_row(rng, qw, qv, c, total, others_pool, mass):
    """a BowVector of `total` words: c of the query's words, holding `mass` of the vector with values near the query's, and total - c words from
    others_pool (disjoint from the query)"""
    pick = np.sort(rng.choice(len(qw), c, replace=False)) if c else np.zeros(0, np.int64)
    cw = qw[pick]
    cv = qv[pick] * rng.uniform(0.8, 1.2, c)
    ow = rng.choice(others_pool, total - c, replace=False)
    ov = rng.random(total - c) + 0.05
    if c and total > c:
        cv, ov = cv / cv.sum() * mass, ov / ov.sum() * (1.0 - mass)
    w = np.concatenate([cw, ow]).astype(np.uint32)
    v = np.concatenate([cv, ov])
    o = np.argsort(w)
    v = v[o] / v[o].sum()
    return w[o], v


def scene(seed, n_words=4096, stride=129, q_stride=129, covis_cap=10, n_filler=20):
    """Three queries over one database.  Query 0 has a loop place whose rows are planted to reach every branch of the census; query 1 sees a place
    of its own but asks for a min_score nothing reaches (status 3); query 2 shares no word with any row (status 1).  Word ids: the queries draw
    from [0, n_words / 2), the rows' other words from [n_words / 2, n_words - 64), query 2 from the last 64 ids."""
    rng = np.random.default_rng(seed)
    half = n_words // 2
    nq = 100
    qws, qvs = [], []
    pool = rng.permutation(half)
    for q in range(2):
        qws.append(np.sort(pool[q * nq:(q + 1) * nq]).astype(np.uint32))     # queries 0 and 1 are disjoint
        qvs.append(normalised(rng, nq))
    qws.append(np.arange(n_words - 64, n_words - 24, dtype=np.uint32))
    qvs.append(normalised(rng, 40))
    others = np.arange(half, n_words - 64)
    rows, tags = [], []

    def add(tag, q, c, total, mass):
        rows.append(planted_row(rng, qws[q], qvs[q], c, total, others, mass))
        tags.append(tag)
        return len(rows) - 1

    # query 0's neighbourhood, rejected: more common words than any candidate
    near = [add("near", 0, c, 120, 0.9) for c in (100, 95, 90)]
    # its loop place: 80 common words is the candidates' maximum -> thr = (unsigned)(0.8f * 80) = 64
    top = add("top", 0, 80, 110, 0.95)
    strong = [add("strong", 0, c, 110, m) for c, m in ((78, 0.9), (75, 0.85), (70, 0.8))]
    dup = [add("dup", 0, 72, 110, 0.97)]
    rows.append(rows[dup[0]]); tags.append("dup"); dup.append(len(rows) - 1)          # the same vector twice: a tie in score
    low = add("low", 0, 66, 110, 0.45)            # kept, but below both duplicates
    weak = add("weak", 0, 70, 129, 0.12)          # above thr, below min_score: adds to totals without being kept
    at_thr = add("at_thr", 0, 64, 110, 0.9)       # common == thr: excluded
    above_thr = add("above_thr", 0, 65, 110, 0.9)  # common == thr + 1
    dead = add("dead", 0, 85, 110, 0.9)           # erased
    lone = add("lone", 0, 68, 110, 0.6)           # a second place of one key frame: kept, total far below 0.75 best_total
    below = [add("below", 0, c, 100, 0.7) for c in (50, 30, 1)]
    # query 1's place
    place1 = [add("place1", 1, c, 110, 0.9) for c in (60, 55, 52)]
    for _ in range(n_filler):                      # unrelated key frames: chance overlaps only
        n = int(rng.integers(60, stride + 1))
        w = np.sort(rng.choice(np.arange(0, n_words - 64), n, replace=False)).astype(np.uint32)
        rows.append((w, normalised(rng, n))); tags.append("filler")
    edge = len(rows)
    rows.append((np.zeros(0, np.uint32), np.zeros(0))); tags.append("empty")
    N = len(rows)
    order = rng.permutation(N)                     # rows in no particular order
    inv = np.argsort(order)
    S = dict(n_words=n_words, db_word=np.zeros((N, stride), np.uint32), db_value=np.zeros((N, stride)), db_n=np.zeros(N, np.int32),
             db_alive=np.ones(N, np.uint8), covis=np.zeros((N, covis_cap), np.int32), n_covis=np.zeros(N, np.int32),
             q_word=np.zeros((3, q_stride), np.uint32), q_value=np.zeros((3, q_stride)), q_n=np.zeros(3, np.int32),
             reject=np.zeros((3, N), np.uint8), min_score=np.array([0.3, 2.0, 0.0], np.float32), tags=[None] * N)
    for i, (w, v) in enumerate(rows):
        r = inv[i]
        S["db_word"][r, :len(w)], S["db_value"][r, :len(w)], S["db_n"][r], S["tags"][r] = w, v, len(w), tags[i]
    for q in range(3):
        S["q_word"][q, :len(qws[q])], S["q_value"][q, :len(qws[q])], S["q_n"][q] = qws[q], qvs[q], len(qws[q])
    R = lambda i: int(inv[i])
    S["db_alive"][R(dead)] = 0
    for i in near:
        S["reject"][0, R(i)] = 1
    S["reject"][1, R(place1[2])] = 1
    S["reject"][2, R(edge)] = 1

    def covis(i, lst):
        lst = lst[:covis_cap]
        S["covis"][R(i), :len(lst)] = [R(j) for j in lst]
        S["n_covis"][R(i)] = len(lst)
    covis(top, [strong[0], weak, dead, strong[1]])
    covis(strong[0], [strong[1], top, weak])                    # best_kf = top
    covis(strong[1], [top, strong[0], dead, at_thr])            # best_kf = top again
    covis(strong[2], [strong[2], strong[1]])                    # names itself: its own score is added once more
    covis(low, [dup[0], dup[1], below[0]])                      # a tie: the first duplicate wins
    covis(dup[0], [low])
    covis(above_thr, [at_thr, weak, dead, below[0], below[1], below[2], low, dup[1], near[0], strong[2]])   # a full list, mostly of rows that add nothing
    covis(weak, [top])
    covis(place1[0], [place1[1], place1[2]])
    covis(near[0], [near[1], near[2]])
    return S


def remapped(S, offset, n_words):
    """the same scene with every word id moved up by offset (order kept): for the count path above the bitmap's limit"""
    T = dict(S)
    T["n_words"] = n_words
    for k in ("db_word", "q_word"):
        T[k] = (S[k] + np.uint32(offset)).astype(np.uint32)
    return T


def census(S, R):
    """how often the restatement's results R on scene S reach each branch the tests must not miss (query by query, summed)"""
    Q, N = R["common"].shape
    c = dict.fromkeys(("rejected_above_all_candidates", "common_eq_thr", "common_eq_thr_plus_1", "score_below_min_score", "covis_added_not_kept",
                       "best_kf_not_self", "shared_best_kf", "kept_total_at_most_075_best", "status_1", "status_3", "dead_row_in_covis",
                       "covis_score_tie_first_wins"), 0)
    for q in range(Q):
        common, rej, ms = R["common"][q].astype(np.int64), S["reject"][q].astype(bool), S["min_score"][q]
        st = int(R["status"][q])
        c["status_1"] += st == 1
        c["status_3"] += st == 3
        cand = (common > 0) & ~rej
        if not cand.any():
            continue
        thr = int(f32(f32(0.8) * f32(common[cand].max())))
        c["rejected_above_all_candidates"] += int(((common > common[cand].max()) & rej).sum())
        c["common_eq_thr"] += int((cand & (common == thr)).sum())
        c["common_eq_thr_plus_1"] += int((cand & (common == thr + 1)).sum())
        sel = cand & (common > thr)
        c["score_below_min_score"] += int((sel & (R["score"][q] < ms)).sum())
        if st != 0:
            continue
        kept = R["best_kf"][q] >= 0
        c["best_kf_not_self"] += int((kept & (R["best_kf"][q] != np.arange(N))).sum())
        bk = R["best_kf"][q][kept]
        c["shared_best_kf"] += int(len(bk) - len(set(bk.tolist())))
        c["kept_total_at_most_075_best"] += int((kept & (R["total"][q] <= f32(f32(0.75) * R["best_total"][q]))).sum())
        for k in np.flatnonzero(kept):
            lst = S["covis"][k][:S["n_covis"][k]]
            c["dead_row_in_covis"] += int(sum(not S["db_alive"][j] for j in lst))
            c["covis_added_not_kept"] += int(sum(bool(sel[j]) and not kept[j] for j in lst))
            b = int(R["best_kf"][q][k])
            if b != k and b in lst.tolist():
                first = lst.tolist().index(b)
                c["covis_score_tie_first_wins"] += int(any(sel[j] and j != b and R["score"][q][j] == R["score"][q][b] for j in lst[first + 1:]))
    return c
