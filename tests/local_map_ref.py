"""The local map of one frame, restated from DESIGN.md section 5, D18, line by line against module::local_map_updater
(module/local_map_updater.cc:60-273) and tracking_module::update_local_map / search_local_landmarks (tracking_module.cc:837-946).

Plain Python over lists, dicts and sets: no numpy in the arithmetic, nothing shared with the library.  `update_local_map` returns the full lists
(no cap); `expected` cuts them to a call's caps and fills what the library leaves unwritten with the caller's sentinel.  Every branch taken is
recorded in the set `ev` (the census of tests/test_local_map_cpu.py reads it)."""
import numpy as np

OK, NO_KEYFRAMES, KF_OVERFLOW, LM_OVERFLOW, LINE_OVERFLOW = range(5)


def tables(scene):
    """the map snapshot of a scene (numpy arrays, the library's layout) as Python lists"""
    t = {}
    for k, v in scene.items():
        t[k] = v.tolist() if isinstance(v, np.ndarray) else v
    F, L = len(t["kf_parent"]), len(t["obs_offsets"]) - 1
    t["F"], t["L"], t["LL"] = F, L, (scene["LL"] if t.get("kf_lm_lines") is not None else 0)
    t["T"], t["C"] = len(t["obs_kf"]), len(t["kf_children"])
    return t


def _cut(c, cap):
    return 0 if c < 0 else cap if c > cap else c


def _run(offsets, row, n):
    lo, hi = offsets[row], offsets[row + 1]
    lo = 0 if lo < 0 else n if lo > n else lo
    hi = lo if hi < lo else n if hi > n else hi
    return lo, hi


def _clean(slots, rows, erased, ev, tag):
    """tracking_module.cc:840-870: a slot whose landmark is erased counts as empty; so does a row outside the table (D18)"""
    out = []
    for lm in slots:
        if lm < 0 or lm >= rows:
            if lm != -1:
                ev.add("out_of_table_" + tag)
            out.append(None)
        elif erased is not None and erased[lm]:
            ev.add("erased_in_" + tag)
            out.append(None)
        else:
            out.append(lm)
    return out


def update_local_map(t, frm_lm, frm_lm_lines, max_num_local_keyfrms=60, ev=None):
    """t: tables(scene); frm_lm / frm_lm_lines: the frame's slots below its count (frm_lm_lines None = the frame holds no line).  Returns
    dict(found, first, weights (of the first), second, nearest, local_lm, held, local_lines, held_lines)."""
    ev = set() if ev is None else ev
    F, L, LL, T, C = t["F"], t["L"], t["LL"], t["T"], t["C"]
    kf_erased = t.get("kf_erased") or [0] * F
    slots = _clean(frm_lm, L, t.get("lm_erased"), ev, "frm_lm")

    # count_keyframe_weights, :89-108
    weights = {}
    seen = set()
    for lm in slots:
        if lm is None:
            continue
        if lm in seen:
            ev.add("held_twice")
        seen.add(lm)
        lo, hi = _run(t["obs_offsets"], lm, T)
        for o in range(lo, hi):
            kf = t["obs_kf"][o]
            if kf < 0 or kf >= F:
                ev.add("out_of_table_obs_kf")
                continue
            weights[kf] = weights.get(kf, 0) + 1
    if not weights:                                   # :78-81
        ev.add("no_keyframes")
        return dict(found=False)

    # find_first_local_keyframes, :110-141, in ascending row (D18)
    first, local, nearest, max_weight = [], set(), -1, 0
    for kf in sorted(weights):
        if kf_erased[kf]:
            continue
        first.append(kf)
        local.add(kf)
        if max_weight < weights[kf]:
            max_weight = weights[kf]
            nearest = kf
    if not first:
        ev.add("every_voted_erased")
    else:
        gone = [weights[kf] for kf in weights if kf_erased[kf]]
        if gone and max(gone) > max_weight:
            ev.add("erased_heaviest")
        if sum(1 for kf in first if weights[kf] == max_weight) > 1:
            ev.add("tie_for_nearest")

    # find_second_local_keyframes, :143-204
    second, how = [], {}

    def add(kf, tag):
        if kf < 0 or kf >= F:                          # !keyfrm
            ev.add(tag + ("_none" if kf == -1 else "_out_of_table"))
            return False
        if kf_erased[kf]:
            ev.add(tag + "_erased")
            return False
        if kf in local:
            ev.add(tag + "_local")
            if tag == "covis" and how.get(kf) == "child":
                ev.add("child_then_covis")
            return False
        local.add(kf)
        second.append(kf)
        how[kf] = tag
        return True

    cut = None
    for i, kf in enumerate(first):
        if max_num_local_keyfrms < len(first) + len(second):
            cut = i
            break
        if max_num_local_keyfrms == len(first) + len(second):
            ev.add("cut_exactly_at_max_still_runs")
        row = t["kf_covis"][kf]
        for j in range(10):
            if add(row[j], "covis"):
                ev.add("covis_first" if j == 0 else "covis_later")
                break
        else:
            ev.add("covis_all_rejected")
        lo, hi = _run(t["kf_children_offsets"], kf, C)
        long_rejected = False
        for o in range(lo, hi):
            if add(t["kf_children"][o], "child"):
                ev.add("child_added")
                if o - lo >= 64:                       # the wide census of tests/test_local_map_wide_cpu.py: runs past one wave of 64
                    ev.add("child_added_at_64_or_later")
                if o - lo >= 128:
                    ev.add("child_added_at_128_or_later")
                break
        else:
            if hi > lo:
                ev.add("children_all_rejected")
            if hi - lo > 64:
                ev.add("children_all_rejected_over_64")
                long_rejected = True
            if hi - lo >= 200:
                ev.add("children_all_rejected_over_200")
        p = t["kf_parent"][kf]
        took = add(p, "parent")
        ev.add("parent_added" if took else "parent_minus_one" if p == -1 else "parent_rejected")
        if took and long_rejected:
            ev.add("parent_added_after_over_64_rejected")
    if first:
        ev.add("cut_never" if cut is None else "cut_at_first_iteration" if cut == 0 else "cut_mid_list")
        if cut is not None and len(first) > 512:
            ev.add("cut_with_over_512_first")

    # find_local_landmarks[_line], :206-273, and the held byte, tracking_module.cc:911-946
    def landmarks(kf_lm, counts, cap, rows, erased, frame_slots, tag):
        out, got = [], set()
        for kf in first + second:
            n = cap if counts is None else _cut(counts[kf], cap)
            inside = set()
            for idx in range(n):
                lm = kf_lm[kf][idx]
                if lm < 0 or lm >= rows:
                    if lm != -1:
                        ev.add("out_of_table_" + tag)
                    continue
                if erased is not None and erased[lm]:
                    ev.add("erased_in_" + tag)
                    continue
                if lm in got:
                    ev.add(("duplicate_inside_" if lm in inside else "duplicate_across_") + tag)
                    continue
                got.add(lm)
                inside.add(lm)
                out.append(lm)
        holds = set(lm for lm in frame_slots if lm is not None)
        held = [1 if lm in holds else 0 for lm in out]
        for h in held:
            ev.add(("held_" if h else "not_held_") + tag)
        return out, held

    r = dict(found=True, first=first, weights=[weights[kf] for kf in first], second=second, nearest=nearest)
    r["local_lm"], r["held"] = landmarks(t["kf_lm"], t.get("kf_counts"), t["cap"], L, t.get("lm_erased"), slots, "kf_lm")
    if t.get("kf_lm_lines") is not None:
        ls = [] if frm_lm_lines is None else _clean(frm_lm_lines, LL, t.get("lm_erased_lines"), ev, "frm_lm_lines")
        r["local_lines"], r["held_lines"] = landmarks(t["kf_lm_lines"], t.get("kf_kl_counts"), t["lcap"], LL, t.get("lm_erased_lines"), ls, "kf_lm_lines")
    return r


def frame_slots(scene, b, lines=False):
    """the slots of frame b below its count, as the reference's loops see them"""
    lm = scene["frm_lm_lines" if lines else "frm_lm"]
    if lm is None:
        return None
    fcap = scene["flcap" if lines else "fcap"]
    cn = scene.get("frm_kl_counts" if lines else "frm_counts")
    n = fcap if cn is None else _cut(int(cn[b]), fcap)
    return lm[b, :n].tolist()


def run_scene(scene, max_num_local_keyfrms=60, ev=None):
    """the restatement of every frame of a scene: a list of update_local_map results"""
    t = tables(scene)
    return [update_local_map(t, frame_slots(scene, b), frame_slots(scene, b, True), max_num_local_keyfrms, ev) for b in range(scene["frm_lm"].shape[0])]


def status_of(r, k_cap, m_cap, ml_cap):
    if not r["found"]:
        return NO_KEYFRAMES
    if len(r["first"]) + len(r["second"]) > k_cap:
        return KF_OVERFLOW
    if len(r["local_lm"]) > m_cap:
        return LM_OVERFLOW
    if "local_lines" in r and len(r["local_lines"]) > ml_cap:
        return LINE_OVERFLOW
    return OK


SENTINEL = dict(status=0xEE, num_first=-77, num_kf=-77, local_kf=-77, first_weight=-77, nearest_kf=-77, num_lm=-77, local_lm=-77, held=0xEE,
                num_lines=-77, local_lines=-77, held_lines=0xEE)
DTYPE = dict(status=np.uint8, held=np.uint8, held_lines=np.uint8)


def expected(results, k_cap, m_cap, ml_cap, lines):
    """the outputs of a call with these caps over sentinel-filled arrays: what D18 says is written, the sentinel everywhere else"""
    B = len(results)
    shape = dict(local_kf=k_cap, first_weight=k_cap, local_lm=m_cap, held=m_cap, local_lines=ml_cap, held_lines=ml_cap)
    names = [k for k in SENTINEL if lines or not k.endswith("lines")]
    o = {k: np.full((B, shape[k]) if k in shape else (B,), SENTINEL[k], DTYPE.get(k, np.int32)) for k in names}
    for b, r in enumerate(results):
        st = status_of(r, k_cap, m_cap, ml_cap)
        o["status"][b] = st
        if st == NO_KEYFRAMES:                          # every count 0, no list row written
            o["num_first"][b] = o["num_kf"][b] = o["num_lm"][b] = 0
            o["nearest_kf"][b] = -1
            if lines:
                o["num_lines"][b] = 0
            continue
        kfs = r["first"] + r["second"]
        wts = r["weights"] + [0] * len(r["second"])
        o["num_first"][b], o["num_kf"][b], o["nearest_kf"][b] = len(r["first"]), len(kfs), r["nearest"]
        for i in range(min(len(kfs), k_cap)):
            o["local_kf"][b, i] = kfs[i]
            o["first_weight"][b, i] = wts[i]
        if st == KF_OVERFLOW:                           # the landmark lists are not written, their counts are 0
            o["num_lm"][b] = 0
            if lines:
                o["num_lines"][b] = 0
            continue
        sides = [("num_lm", "local_lm", "held", m_cap)] + ([("num_lines", "local_lines", "held_lines", ml_cap)] if lines else [])
        for num, lst, held, cap in sides:
            o[num][b] = len(r[lst])
            for i in range(min(len(r[lst]), cap)):
                o[lst][b, i] = r[lst][i]
                o[held][b, i] = r[held][i]
    return o
