"""Plane creation for G key frames on one stream, without the host: instance masks, key points and the shared landmark tables in, fitted planes
and a landmark-to-plane table out.

`plane_step.run` does what Planar_Mapping_module::create_ColorToPlane (planar_mapping_module.cc:185-345) and create_new_plane (:347-410) do per
key frame, up to the objects:

  1  valid        a key point votes when it has a landmark that is neither erased nor owned by a plane (:208); torch ops on the landmark tables
  2  plp_color_vote_device                the colour label under every such key point (:219-330)
  3  group        the key points of a key frame by label: a stable sort by label and the run boundaries, torch ops of static shape (no .item(),
                  no copy to the host, no boolean-mask indexing).  A key frame has at most c_cap labels; plane row g * c_cap + c is the c-th
                  label of key frame g in ASCENDING label order, its slots are the label's key points in KEY-POINT order.  Both orders are by
                  definition: colorToPlanes is an unordered_map and get_landmarks() iterates one.  Rows
                  beyond a key frame's number of labels have counts = 0; labels beyond c_cap are dropped (num_labels reports them)
  4  gather       the slots' positions and flag bytes from the landmark tables
  5  plp_plane_ransac_device(PLP_PLANE_CREATE)     the gate (:359) and estimate_plane_sequential_RANSAC (:412-591) for all G * c_cap rows
  6  tables       lm_plane [L] i32: the plane row that took the landmark in step [4] of a PLANE_OK row, else -1 (where two rows take one
                  landmark -- it is observed in two of the G key frames -- the higher row wins; the reference would have given it to the key
                  frame it visits first and marked it owned); equation [G * c_cap, 4] and active [G * c_cap] u8 (PLANE_OK and at least
                  points_per_ransac members), which plp_plane_refine_points_device reads

What stays on the host: new data::Plane, set_landmarks / the ownership writes of a new plane, add_landmark_plane /
erase_landmark_plane.  merge_planes, refine_planes and refine_points over the map's plane table are plane_refinement_step.py, which appends this
step's rows to that table.

Tables are torch tensors on the step's device:
  key frames  mask [G, rows, cols, 3] u8, undist [G, cap, 28] u8 (undist_keypts_ as plp_keypoint), counts [G] i32, lm_index [G, cap] i32 (the
              landmark row of a key point, -1: none), dist_thresh / error_thresh [G] f64 (_planar_distance_thresh, _final_error_thresh of the key
              frame's map scale, e.g. from plp_median_depth_device) or numbers
  landmarks   pos_w [L, 3] f64, plane_flags [L] u8 (PLANE_LM_ERASED | PLANE_LM_OWNED)
"""


class plane_step:
    def __init__(self, plp, c_cap=8, points_per_ransac=18, min_points_before_ransac=12, iters=50, inliers_ratio_thr=0.7, check_3x3_window=True,
                 seed=0, device_index=0):
        import torch
        self.torch, self.plp = torch, plp
        self.dev = torch.device("cuda", device_index)
        self.c_cap, self.ppr, self.min_points, self.iters, self.ratio = int(c_cap), int(points_per_ransac), int(min_points_before_ransac), int(iters), float(inliers_ratio_thr)
        self.check, self.seed = bool(check_3x3_window), seed
        self.mt = plp.matcher(device=device_index)

    def run(self, keyframes, landmarks, stream=None, hypotheses=False):
        """Enqueue the step on `stream` (default: the current stream).  Returns dict(labels [G, cap] i32, plane_label [G * c_cap] i32 (0: no
        plane), num_labels [G] i32, counts [G * c_cap] i32, slot_kp / slot_lm [G * c_cap, cap] i32 (-1: no slot), pos_w [G * c_cap, cap, 3],
        flags, the outputs of plp_plane_ransac_device named as in PLANE_RANSAC_OUTPUTS (hyp_* only with hypotheses=True), lm_plane [L] i32,
        active [G * c_cap] u8).  Nothing is synchronised."""
        torch, plp = self.torch, self.plp
        i32, i64, f64, u8 = torch.int32, torch.int64, torch.float64, torch.uint8
        st = stream or torch.cuda.current_stream(self.dev)
        mask, undist, counts, lm_index = keyframes["mask"], keyframes["undist"], keyframes["counts"], keyframes["lm_index"]
        pos_w, lm_flags = landmarks["pos_w"], landmarks["plane_flags"]
        G, rows, cols = mask.shape[0], mask.shape[1], mask.shape[2]
        cap, L, Cc = undist.shape[1], pos_w.shape[0], self.c_cap
        P = G * Cc
        if cap > 8192:
            raise plp.PlpError(plp.PLP_ERR_UNSUPPORTED, "more than 8192 key points per key frame")
        with torch.cuda.stream(st):
            # 1: who votes
            lm = lm_index.to(i64)
            has = (lm >= 0) & (lm < L)
            lmc = lm.clamp(0, max(L - 1, 0))
            fl = lm_flags[lmc] if L else torch.zeros_like(lm, dtype=u8)
            valid = (has & (fl == 0)).to(u8).contiguous()
            labels = torch.zeros((G, cap), dtype=i32, device=self.dev)
        # 2: the vote
        plp._check(plp.lib().plp_color_vote_device(self.mt._h, mask.data_ptr(), rows, cols, cols * 3, rows * cols * 3, undist.data_ptr(), valid.data_ptr(),
                                                  counts.data_ptr(), cap, G, int(self.check), labels.data_ptr(), st.cuda_stream))
        with torch.cuda.stream(st):
            # 3: runs of equal labels after a stable sort; label 0 (no vote) sorts behind every label
            none = torch.iinfo(torch.int64).max
            key = torch.where(labels != 0, labels.to(i64), torch.full((G, cap), none, dtype=i64, device=self.dev))
            skey, order = torch.sort(key, dim=1, stable=True)
            first = torch.ones((G, cap), dtype=torch.bool, device=self.dev)
            first[:, 1:] = skey[:, 1:] != skey[:, :-1]
            run = torch.cumsum(first.to(i64), 1) - 1                              # the run a sorted position belongs to
            voted = skey != none
            num_labels = (first & voted).sum(1).to(i32)
            kept = voted & (run < Cc)
            idx = torch.arange(cap, device=self.dev, dtype=i64).expand(G, cap)
            start = torch.cummax(torch.where(first, idx, torch.zeros_like(idx)), 1).values   # where the run of a position begins
            slot = idx - start
            g = torch.arange(G, device=self.dev, dtype=i64).unsqueeze(1).expand(G, cap)
            row = torch.where(kept, g * Cc + run, torch.full_like(run, P))        # row P takes what is dropped
            counts_p = torch.zeros(P + 1, dtype=i32, device=self.dev).index_add_(0, row.reshape(-1), torch.ones(G * cap, dtype=i32, device=self.dev))[:P]
            plane_label = torch.zeros(P + 1, dtype=i32, device=self.dev)
            plane_label[row.reshape(-1)] = torch.where(kept, skey, torch.zeros_like(skey)).to(i32).reshape(-1)   # equal values within a row
            plane_label = plane_label[:P]
            slot_kp = torch.full((P + 1, cap), -1, dtype=i32, device=self.dev)
            slot_kp[row.reshape(-1), slot.reshape(-1)] = order.to(i32).reshape(-1)   # (row, slot) pairs are distinct below row P
            slot_kp = slot_kp[:P].contiguous()
            # 4: the slots' landmarks
            have = slot_kp >= 0
            kp = slot_kp.to(i64).clamp(0)
            gp = (torch.arange(P, device=self.dev, dtype=i64) // Cc).unsqueeze(1)
            slot_lm = torch.where(have, lm_index[gp, kp], torch.full_like(slot_kp, -1))
            lms = slot_lm.to(i64).clamp(0, max(L - 1, 0))
            p_pos = (pos_w[lms] if L else torch.zeros((P, cap, 3), dtype=f64, device=self.dev)).contiguous()
            p_flags = torch.where(have, lm_flags[lms] if L else torch.zeros_like(slot_kp, dtype=u8), torch.full_like(slot_kp, plp.PLANE_LM_ERASED, dtype=u8)).contiguous()

            def per_plane(v):
                t = v if torch.is_tensor(v) else torch.full((G,), float(v), dtype=f64, device=self.dev)
                return t.to(f64).reshape(G, 1).expand(G, Cc).reshape(P).contiguous()
            d_thr, e_thr = per_plane(keyframes["dist_thresh"]), per_plane(keyframes["error_thresh"])
            out = {}
            for k, (shape, dt, optional) in plp.PLANE_RANSAC_OUTPUTS.items():
                if optional and not hypotheses:
                    continue
                out[k] = torch.zeros((P,) + shape(cap, self.iters), dtype=getattr(torch, dt.__name__), device=self.dev)
        # 5: the fits
        self.mt.plane_ransac_device(plp.PLANE_CREATE, P, cap, p_pos, p_flags, d_thr, e_thr, out, points_per_ransac=self.ppr,
                                    min_points_before_ransac=self.min_points, iters=self.iters, inliers_ratio_thr=self.ratio, seed=self.seed,
                                    counts=counts_p, stream=st)
        with torch.cuda.stream(st):
            # 6: the tables
            ok = out["status"] == plp.PLANE_OK
            member = have & (out["inliers"] == 1) & ok.unsqueeze(1)
            rows_p = torch.arange(P, device=self.dev, dtype=i32).unsqueeze(1).expand(P, cap)
            lm_plane = torch.full((L + 1,), -1, dtype=i32, device=self.dev)
            lm_plane.scatter_reduce_(0, torch.where(member, slot_lm.to(i64), torch.full_like(lms, L)).reshape(-1),
                                     torch.where(member, rows_p, torch.full_like(rows_p, -1)).reshape(-1), "amax")
            active = (ok & (out["num_inliers"] >= self.ppr)).to(u8)
        res = dict(labels=labels, plane_label=plane_label, num_labels=num_labels, counts=counts_p, slot_kp=slot_kp, slot_lm=slot_lm, pos_w=p_pos,
                   flags=p_flags, lm_plane=lm_plane[:L], active=active)
        res.update(out)
        return res
