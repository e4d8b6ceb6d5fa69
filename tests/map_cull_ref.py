"""A plain restatement of module::local_map_cleaner (module/local_map_cleaner.cc:51-320) at object level, for DESIGN.md section 5, D20: small
key-frame and landmark objects with an observation dict and num_observations_, the real mutation of keyframe::prepare_for_erasing
(keyframe.cc:872-926), landmark::erase_observation (landmark.cc:99-136), landmark::prepare_for_erasing (:365-383) and
keyframe::erase_landmark_with_index, and the reference's loops run one after the other on a copy of the map.  The library computes the
closed form of D20 instead (a set of removed key frames, no per-landmark state); the tests hold one against the other.

`events`, where given, collects what a run came through, for the census of tests/test_map_cull_cpu.py."""
import numpy as np

SKIP_ORIGIN, SKIP_WINDOW, KEPT, REMOVED, REMOVED_HELD, ABSENT = range(6)
HOLD, DROP, ERASE = range(3)
# what the tests fill the outputs with before a call: a value no call writes
SENTINEL = dict(num_removed=-77, decision=0xEE, num_valid=-77, num_redundant=-77, kf_removed=0xEE, lm_erased=0xEE,
                state=0xEE, num_fresh=-77, fresh=-77)


class Landmark:
    def __init__(self, row):
        self.row, self.observations, self.num_observations, self.will_be_erased = row, {}, 0, False

    def add_observation(self, kf, idx):                      # landmark.cc:80-97
        if kf in self.observations:
            return
        self.observations[kf] = idx
        self.num_observations += 2 if 0 <= kf.x_right[idx] else 1

    def erase_observation(self, kf):                         # :99-136
        discard = False
        if kf in self.observations:
            idx = self.observations[kf]
            self.num_observations = (self.num_observations - (2 if 0 <= kf.x_right[idx] else 1)) & 0xFFFFFFFF
            del self.observations[kf]
            if self.num_observations <= 2:
                discard = True
        if discard:
            self.prepare_for_erasing()

    def prepare_for_erasing(self):                           # :365-383
        observations, self.observations, self.will_be_erased = self.observations, {}, True
        for kf, idx in observations.items():
            kf.landmarks[idx] = None                         # erase_landmark_with_index


class Keyframe:
    def __init__(self, row, id_, octaves, x_right, depths, depth_thr, cannot_be_erased):
        self.row, self.id, self.octaves, self.x_right, self.depths, self.depth_thr = row, id_, octaves, x_right, depths, depth_thr
        self.cannot_be_erased, self.landmarks, self.removed_now = cannot_be_erased, [], False

    def prepare_for_erasing(self, origin_id):                # keyframe.cc:872-926, the part that touches what the loop reads
        if self.id == origin_id or self.cannot_be_erased:
            return
        self.removed_now = True
        for lm in self.landmarks:
            if lm is not None:
                lm.erase_observation(self)


def build_map(sc):
    """the objects of a scene's tables (tests/map_cull_scene.py); a row outside its table is no object (D20's row checks)"""
    F, cap = sc["kf_lm"].shape
    L = len(sc["obs_offsets"]) - 1
    stride = sc["undist"].shape[1]
    xr = sc["x_right"] if sc["x_right"] is not None else np.full((F, stride), -1.0, np.float32)
    kfs = [Keyframe(f, int(sc["kf_id"][f]), sc["undist"]["octave"][f], xr[f], None if sc["depths"] is None else sc["depths"][f],
                    None if sc["depth_thr"] is None else sc["depth_thr"][f], bool(sc["kf_cannot_erase"] is not None and sc["kf_cannot_erase"][f]))
           for f in range(F)]
    lms = [Landmark(l) for l in range(L)]
    for l, lm in enumerate(lms):
        lm.will_be_erased = bool(sc["lm_erased"] is not None and sc["lm_erased"][l])
        for t in range(int(sc["obs_offsets"][l]), int(sc["obs_offsets"][l + 1])):
            kf, idx = int(sc["obs_kf"][t]), int(sc["obs_idx"][t])
            if 0 <= kf < F and 0 <= idx < cap:
                lm.add_observation(kfs[kf], idx)
        if sc["lm_num_obs"] is not None:
            lm.num_observations = int(sc["lm_num_obs"][l])
    for f, kf in enumerate(kfs):
        n = cap if sc["kf_counts"] is None else min(max(int(sc["kf_counts"][f]), 0), cap)
        kf.landmarks = [lms[v] if 0 <= v < L else None for v in (int(x) for x in sc["kf_lm"][f, :n])]
    return kfs, lms


def count_redundant_observations(kf, is_monocular, events=None):     # local_map_cleaner.cc:242-320
    num_valid = num_redundant = 0
    for idx, lm in enumerate(kf.landmarks):
        if lm is None or lm.will_be_erased:
            continue
        if not is_monocular:
            depth = kf.depths[idx]
            if depth < np.float32(0.0) or kf.depth_thr < depth:
                if events is not None:
                    events.add("depth_negative" if depth < 0 else "depth_above_thr")
                continue
            if events is not None and np.isnan(depth):
                events.add("depth_nan")
        num_valid += 1
        if events is not None and lm.num_observations in (3, 4):
            events.add(f"num_observations_{lm.num_observations}")
        if lm.num_observations <= 3:
            continue
        scale_level = int(kf.octaves[idx])
        num_better, redundant = 0, False
        obs = list(lm.observations.items())
        for i, (ngh, ngh_idx) in enumerate(obs):
            if ngh.row == kf.row:
                continue
            if int(ngh.octaves[ngh_idx]) <= scale_level + 1:
                num_better += 1
                if 3 <= num_better:
                    redundant = True
                    if events is not None and i == len(obs) - 1:
                        events.add("third_better_is_last")
                    break
        num_redundant += redundant
    return num_valid, num_redundant


def decide(num_valid, num_redundant):
    """:232 in float: 0 / 0 is NaN and keeps the key frame"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool(np.float32(0.9) <= np.float32(num_redundant) / np.float32(num_valid))


def remove_redundant_keyframes(sc, g, events=None):
    """problem g of a scene on its own copy of the map: dict(num_removed, entries: one (decision, num_valid, num_redundant) per entry of the
    problem's list (the counts None when skipped), kf_removed [F], lm_erased [L])"""
    kfs, lms = build_map(sc)
    pristine = build_map(sc)[0] if events is not None else None       # for the census: what the snapshot's counts alone would decide
    F, mono, origin = len(kfs), bool(sc["is_monocular"]), int(sc["origin_id"])
    cur = int(sc["cur_kf"][g])
    lo, hi = int(sc["covis_offsets"][g]), int(sc["covis_offsets"][g + 1])
    entries, num_removed = [], 0
    for c in (int(v) for v in sc["covis"][lo:hi]):
        if not (0 <= c < F and 0 <= cur < F):
            entries.append((ABSENT, None, None))
            continue
        kf, id_cur = kfs[c], kfs[cur].id
        if kf.id == origin:
            entries.append((SKIP_ORIGIN, None, None))
            continue
        in_window = kf.id <= id_cur and id_cur <= ((kf.id + 2) & 0xFFFFFFFF)
        if events is not None:
            for d, name in ((0, "window_at_cur"), (2, "window_at_cur_minus_2"), (3, "window_below"), (-1, "window_above")):
                if id_cur - kf.id == d:
                    events.add(name + ("_skipped" if in_window else "_counted"))
        if in_window:
            entries.append((SKIP_WINDOW, None, None))
            continue
        nv, nr = count_redundant_observations(kf, mono, events)
        removed = decide(nv, nr)
        if events is not None:
            if sc["kf_erased"] is not None and sc["kf_erased"][c]:
                events.add("erased_keyframe_in_list")
            if nv == 0:
                events.add("num_valid_0")
            if (nr, nv) in ((9, 10), (8, 9)):
                events.add(f"ratio_{nr}_{nv}_" + ("removed" if removed else "kept"))
            snv, snr = count_redundant_observations(pristine[c], mono)
            if snv != nv:
                events.add("cascade_changes_num_valid")
            if decide(snv, snr) != removed:
                events.add("flip_to_removed" if removed else "flip_to_kept")
        if removed:
            num_removed += 1
            held = kf.cannot_be_erased
            kf.prepare_for_erasing(origin)
            entries.append((REMOVED_HELD if held else REMOVED, nv, nr))
        else:
            entries.append((KEPT, nv, nr))
    if events is not None:
        events.update(("SKIP_ORIGIN", "SKIP_WINDOW", "KEPT", "REMOVED", "REMOVED_HELD", "ABSENT")[e[0]] for e in entries)
        if sum(e[0] == REMOVED for e in entries) >= 2:
            events.add("two_removals")
    return dict(num_removed=num_removed, entries=entries, kf_removed=np.array([k.removed_now for k in kfs], np.uint8),
                lm_erased=np.array([l.will_be_erased for l in lms], np.uint8))


def expected_keyframes(results, sc, optional=True):
    """the output arrays of plp_cull_keyframes_* for the scene's problems over sentinel-filled arrays"""
    G, Cv = len(results), len(sc["covis"])
    F, L = sc["kf_lm"].shape[0], len(sc["obs_offsets"]) - 1
    o = dict(num_removed=np.array([r["num_removed"] for r in results], np.int32).reshape(G),
             decision=np.full(Cv, SENTINEL["decision"], np.uint8), num_valid=np.full(Cv, SENTINEL["num_valid"], np.int32),
             num_redundant=np.full(Cv, SENTINEL["num_redundant"], np.int32))
    for g, r in enumerate(results):
        for j, (d, nv, nr) in enumerate(r["entries"], int(sc["covis_offsets"][g])):
            o["decision"][j] = d
            if nv is not None:
                o["num_valid"][j], o["num_redundant"][j] = nv, nr
    if optional:
        o["kf_removed"] = np.array([r["kf_removed"] for r in results], np.uint8).reshape(G, F)
        o["lm_erased"] = np.array([r["lm_erased"] for r in results], np.uint8).reshape(G, L)
    return o


def remove_redundant_landmarks(sc, r, events=None):
    """list r of a landmark scene, :51-131 / :133-199: (states, the list afterwards, num_removed)"""
    L = len(sc["num_observed"])
    cur, thr = int(sc["cur_kf_id"][r]), int(sc["num_obs_thr"][r])
    fresh = [int(v) for v in sc["fresh"][int(sc["fresh_offsets"][r]):int(sc["fresh_offsets"][r + 1])]]
    states, num_removed = [], 0
    ev = (lambda *a: events.update(a)) if events is not None else (lambda *a: None)
    for lm in fresh:
        state = HOLD
        if not 0 <= lm < L:
            state = DROP
            ev("row_outside")
        else:
            plane = bool(sc["owning_plane"] is not None and sc["owning_plane"][lm])
            first = int(sc["first_kf_id"][lm])
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.float32(sc["num_observed"][lm]) / np.float32(sc["num_observable"][lm])
            if sc["num_observable"][lm] == 0:
                ev("ratio_0_0" if sc["num_observed"][lm] == 0 else "ratio_x_0")
            if sc["lm_erased"] is not None and sc["lm_erased"][lm]:
                state = DROP
                ev("branch_erased")
            elif ratio < np.float32(0.3):
                state = DROP if plane else ERASE
                ev("branch_ratio", "ratio_plane" if plane else "ratio_no_plane")
            elif ((2 + first) & 0xFFFFFFFF) <= cur and int(sc["num_obs"][lm]) <= thr:
                state = DROP if plane else ERASE
                ev("branch_few_observers", "few_plane" if plane else "few_no_plane")
            elif ((3 + first) & 0xFFFFFFFF) <= cur:
                state = DROP
                ev("branch_enough_observers")
            else:
                ev("branch_not_clear")
            if not (sc["lm_erased"] is not None and sc["lm_erased"][lm]) and not ratio < np.float32(0.3):   # the id tests were reached
                if 2 + first == cur:
                    ev("first_plus_2_equals_cur_" + ("few" if int(sc["num_obs"][lm]) <= thr else "many"))
                if 2 + first == cur - 1:
                    ev("first_plus_2_one_below_cur_" + ("few" if int(sc["num_obs"][lm]) <= thr else "many"))
            if sc["owning_plane"] is None:
                ev("line_variant")
        states.append(state)
        num_removed += state == ERASE
    return states, [lm for lm, s in zip(fresh, states) if s == HOLD], num_removed


def expected_landmarks(sc, events=None):
    R, N = len(sc["cur_kf_id"]), len(sc["fresh"])
    o = dict(state=np.full(N, SENTINEL["state"], np.uint8), num_removed=np.zeros(R, np.int32), num_fresh=np.zeros(R, np.int32),
             fresh=np.full(N, SENTINEL["fresh"], np.int32))
    for r in range(R):
        states, kept, n = remove_redundant_landmarks(sc, r, events)
        lo = int(sc["fresh_offsets"][r])
        o["state"][lo:lo + len(states)] = states
        o["fresh"][lo:lo + len(kept)] = kept
        o["num_removed"][r], o["num_fresh"][r] = n, len(kept)
    return o
