"""An object-level restatement of data::graph_node (src/PLPSLAM/data/graph_node.cc:36-285), written from the text line by line: a connected map
(dict), an ordered list and a spanning parent per key frame, mutated one call after another.  It knows nothing of the closed form of DESIGN.md
section 5, D21: the library's tables are held to what these objects become.

Key-frame rows stand in for keyframe*: a std::map over pointers iterates in ascending row, a std::pair<unsigned, keyframe*> compares by weight and
then by row.  `events` collects the names of the cases met, for the census of tests/test_covisibility_cpu.py."""
import numpy as np

OK, NO_SHARED, ROW_ABSENT, DUPLICATE, OVERFLOW = range(5)
WEIGHT_THR = 15                    # weight_thr_ (graph_node.h)
SENTINEL = dict(status=0xEE, nearest=-77, max_weight=-77, touched=0xEE)
SLACK = -77                        # what the tests put behind the last entry of a row before a call


class graph:
    """the graph_node of every key frame of a map"""

    def __init__(self, F):
        self.connected = [dict() for _ in range(F)]          # connected_keyfrms_and_weights_
        self.ordered = [[] for _ in range(F)]                # ordered_covisibilities_
        self.ordered_w = [[] for _ in range(F)]              # ordered_weights_
        self.parent = [-1] * F                               # spanning_parent_
        self.parent_unset = [True] * F                       # spanning_parent_is_not_set_
        self.written = set()                                 # the key frames whose members a call assigned

    def copy(self):
        g = graph(len(self.connected))
        g.connected = [dict(c) for c in self.connected]
        g.ordered, g.ordered_w = [list(o) for o in self.ordered], [list(o) for o in self.ordered_w]
        g.parent, g.parent_unset = list(self.parent), list(self.parent_unset)
        return g

    # :195-219
    def update_covisibility_orders(self, k):
        pairs = [(w, kf) for kf, w in sorted(self.connected[k].items())]
        pairs.sort(reverse=True)                             # std::sort(rbegin, rend): descending (weight, keyframe*)
        self.ordered[k] = [kf for w, kf in pairs]
        self.ordered_w[k] = [w for w, kf in pairs]
        self.written.add(k)

    # :36-59
    def add_connection(self, k, keyfrm, weight, events=None):
        need_update = False
        c = self.connected[k]
        if keyfrm not in c:
            c[keyfrm] = weight
            need_update = True
        elif c[keyfrm] != weight:
            c[keyfrm] = weight
            need_update = True
            if events is not None:
                events.add("back_edge_changes_stale_weight")
        elif events is not None:
            events.add("back_edge_equal_weight")
            if len(self.ordered[k]) < len(c):
                events.add("back_edge_equal_weight_list_stays_thresholded")
        if need_update:
            self.update_covisibility_orders(k)
            if events is not None and self.ordered_w[k] and self.ordered_w[k][-1] <= WEIGHT_THR and len(self.ordered[k]) > 1:
                events.add("rebuilt_list_shows_entries_at_or_below_thr")

    # :61-77
    def erase_connection(self, k, keyfrm):
        need_update = False
        if keyfrm in self.connected[k]:
            del self.connected[k][keyfrm]
            need_update = True
        if need_update:
            self.update_covisibility_orders(k)

    # :79-90
    def erase_all_connections(self, k, events=None):
        for keyfrm in sorted(self.connected[k]):
            if events is not None and k not in self.connected[keyfrm]:
                events.add("erase_target_does_not_hold_me")
            self.erase_connection(keyfrm, k)
        self.connected[k] = {}
        self.ordered[k], self.ordered_w[k] = [], []
        self.written.add(k)

    # :92-193; sc: the map snapshot (kf_lm, kf_counts, obs_offsets, obs_kf, lm_erased, kf_id; T: the length the runs are cut to)
    def update_connections(self, k, sc, events=None):
        ev = events if events is not None else set()
        F, cap = sc["kf_lm"].shape
        L, T = len(sc["obs_offsets"]) - 1, sc.get("T", len(sc["obs_kf"]))
        cnt = cap if sc.get("kf_counts") is None else min(max(int(sc["kf_counts"][k]), 0), cap)
        weights = {}                                         # keyfrm_weights, a std::map
        seen = set()
        for lm in (int(v) for v in sc["kf_lm"][k, :cnt]):   # get_landmarks()
            if lm == -1:
                ev.add("slot_none")
            if not 0 <= lm < L:                              # !lm
                if lm != -1:
                    ev.add("landmark_row_outside_table")
                continue
            if sc.get("lm_erased") is not None and sc["lm_erased"][lm]:   # will_be_erased()
                ev.add("landmark_erased")
                continue
            if lm in seen:
                ev.add("landmark_in_two_slots")
            seen.add(lm)
            lo, hi = int(sc["obs_offsets"][lm]), int(sc["obs_offsets"][lm + 1])
            if hi > T:
                ev.add("run_cut_at_T")
            lo = min(max(lo, 0), T)
            hi = min(max(hi, lo), T)
            for keyfrm in (int(v) for v in sc["obs_kf"][lo:hi]):
                if keyfrm == k:
                    continue
                if not 0 <= keyfrm < F:
                    ev.add("observer_row_outside_table")
                    continue
                weights[keyfrm] = weights.get(keyfrm, 0) + 1
        if not weights:
            ev.add("no_shared")
            return NO_SHARED, -1, 0
        max_weight, nearest = 0, None
        pairs = []
        for keyfrm in sorted(weights):
            weight = weights[keyfrm]
            if max_weight <= weight:
                if max_weight == weight:
                    ev.add("tie_at_max_weight")
                max_weight, nearest = weight, keyfrm
            if WEIGHT_THR < weight:
                pairs.append((weight, keyfrm))
            if WEIGHT_THR - 1 <= weight <= WEIGHT_THR + 2:
                ev.add(f"weight_{weight}")
        if not pairs:
            ev.add("single_node_below_thr")
            pairs.append((max_weight, nearest))
        if len({w for w, kf in pairs}) < len(pairs):
            ev.add("tie_among_pairs")
        for weight, covisibility in pairs:
            self.add_connection(covisibility, k, weight, ev)
        pairs.sort(reverse=True)
        self.connected[k] = weights
        self.ordered[k] = [kf for w, kf in pairs]
        self.ordered_w[k] = [w for w, kf in pairs]
        self.written.add(k)
        if self.parent_unset[k] and int(sc["kf_id"][k]) != 0:
            assert nearest == self.ordered[k][0]
            self.parent[k] = nearest
            self.parent_unset[k] = False
            ev.add("parent_set")
        elif self.parent_unset[k]:
            ev.add("parent_id_0")
        else:
            ev.add("parent_flag_already_clear")
        return OK, nearest, max_weight

    # :221-285
    def get_connected_keyframes(self, k):
        return set(self.connected[k])

    def get_covisibilities(self, k):
        return list(self.ordered[k])

    def get_top_n_covisibilities(self, k, n):
        return list(self.ordered[k]) if len(self.ordered[k]) < n else self.ordered[k][:n]

    def get_covisibilities_over_weight(self, k, weight, events=None):
        if not self.ordered[k]:
            return []
        w = self.ordered_w[k]
        itr = next((i for i, v in enumerate(w) if not v >= weight), len(w))     # std::upper_bound with std::greater
        if itr == len(w):
            if events is not None:
                events.add("over_weight_all_qualify_returns_empty")
            return []
        if events is not None and itr > 0:
            events.add("over_weight_proper_prefix")
        return self.ordered[k][:itr]

    def get_weight(self, k, keyfrm):
        return self.connected[k].get(keyfrm, 0)


def run_update(g, sc, owners, events=None):
    """update_connections() of `owners`, one after another; what the C ABI adds is here: an owner outside the table and an owner met before are
    not processed.  Returns (status, nearest, max_weight) per owner; g.written names the rows a call assigned."""
    F = sc["kf_lm"].shape[0]
    ev = events if events is not None else set()
    g.written = set()
    out, done, pairs_of = [], [], {}
    for k in (int(v) for v in owners):
        if not 0 <= k < F:
            out.append((ROW_ABSENT, -1, 0))
        elif k in done:
            out.append((DUPLICATE, -1, 0))
        else:
            r = g.update_connections(k, sc, ev)
            out.append(r)
            if r[0] == OK:
                pairs_of[k] = set(g.ordered[k])
                for e in done:                               # both positional orders of a mutually covisible pair of owners
                    if e in pairs_of and e in pairs_of[k] and k in pairs_of[e]:
                        ev.add("mutual_owners_low_row_first" if e < k else "mutual_owners_high_row_first")
            else:
                ev.add("__empty:%d" % k)
        done.append(k)
    # an owner without a weight that owners before it and owners after it connect to
    for k in [int(e[8:]) for e in ev if e.startswith("__empty:")]:
        at = done.index(k)
        before = any(k in pairs_of.get(e, ()) for e in done[:at])
        after = any(k in pairs_of.get(e, ()) for e in done[at + 1:])
        if before and after:
            ev.add("empty_owner_receives_before_and_after")
    for e in [e for e in ev if e.startswith("__empty:")]:
        ev.discard(e)
    return out


def run_erase(g, mask, events=None):
    """erase_all_connections() of every key frame of the mask, in ascending row"""
    g.written = set()
    rows = [int(k) for k in np.flatnonzero(mask)]
    if events is not None:
        if len(rows) == 1:
            events.add("erase_one")
        if any(a in g.connected[b] and b in g.connected[a] for a in rows for b in rows if a < b):
            events.add("erase_mutually_connected_pair")
    for k in rows:
        g.erase_all_connections(k, events)
    if events is not None:
        gone = set(rows)
        if any(gone & set(c) for j, c in enumerate(g.connected) if j not in gone):
            events.add("stale_one_sided_entry_survives")


def tables(g, conn_cap, covis_cap, kf_parent_dtype=np.int32):
    """the graph as the tables of plp_covisibility_*: every row whole, -1 / 0 behind the last entry, cut to the caps (the counts are not)"""
    F = len(g.connected)
    t = dict(kf_conn=np.full((F, conn_cap), -1, np.int32), kf_conn_w=np.zeros((F, conn_cap), np.int32), kf_n_conn=np.zeros(F, np.int32),
             kf_covis=np.full((F, covis_cap), -1, np.int32), kf_covis_w=np.zeros((F, covis_cap), np.int32), kf_n_covis=np.zeros(F, np.int32),
             kf_parent=np.array(g.parent, kf_parent_dtype), kf_parent_unset=np.array(g.parent_unset, np.uint8))
    for k in range(F):
        c = sorted(g.connected[k].items())[:conn_cap]
        t["kf_n_conn"][k], t["kf_n_covis"][k] = len(g.connected[k]), len(g.ordered[k])
        t["kf_conn"][k, :len(c)] = [kf for kf, w in c]
        t["kf_conn_w"][k, :len(c)] = [w for kf, w in c]
        o = min(len(g.ordered[k]), covis_cap)
        t["kf_covis"][k, :o] = g.ordered[k][:o]
        t["kf_covis_w"][k, :o] = g.ordered_w[k][:o]
    return t


def with_slack(t):
    """the tables with SLACK behind the last entry of every row: what a call does not write stays visible"""
    t = {k: v.copy() for k, v in t.items()}
    for rows, n in (("kf_conn", "kf_n_conn"), ("kf_conn_w", "kf_n_conn"), ("kf_covis", "kf_n_covis"), ("kf_covis_w", "kf_n_covis")):
        behind = np.arange(t[rows].shape[1])[None, :] >= t[n][:, None]
        t[rows][behind] = SLACK
    return t


def expected_state(before, g, conn_cap, covis_cap, names=None):
    """the tables after a call: the rows the call assigned whole, every other row as `before` holds it"""
    after = tables(g, conn_cap, covis_cap)
    rows = sorted(g.written)
    want = {k: v.copy() for k, v in before.items()}
    for k in (names or before):
        want[k][rows] = after[k][rows]
    return want


def expected_update(res, g, F):
    """the outputs of plp_covisibility_update_* without an overflow"""
    touched = np.zeros(F, np.uint8)
    touched[sorted(g.written)] = 1
    return dict(status=np.array([r[0] for r in res], np.uint8), nearest=np.array([r[1] for r in res], np.int32),
                max_weight=np.array([r[2] for r in res], np.int32), touched=touched)


def expected_erase(g, F):
    touched = np.zeros(F, np.uint8)
    touched[sorted(g.written)] = 1
    return dict(status=np.zeros(F, np.uint8), touched=touched)
