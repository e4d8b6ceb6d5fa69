"""The local map of B tracked frames: the map's tables and the frames' landmark slots in, the per-frame tables of local landmarks that
posed_tracker_step.run_local and tracked_pose_step.run read out, on one stream, without the host.

`local_map_step.run` does what tracking_module::update_local_map (tracking_module.cc:837-906) does between the first pose optimisation and
search_local_landmarks[_line], module::local_map_updater (module/local_map_updater.cc:60-273):

  1  plp_local_map_device   the weights, the first and second local key frames, `nearest`, the local landmarks and lines in first-seen order and
                            the byte that says the frame holds one already                                           :60-273, tracking_module.cc:911-946
  2  torch, on the stream   gathers of static shape [B, m_cap] / [B, ml_cap] from the shared landmark tables into the `local` dict of posed_step.py;
                            ref_keyfrm_ = nearest where there is one (:888-892)

No .item(), no copy to the host, no boolean-mask indexing.  kf_covis, kf_parent and the children lists are covisibility_step's views of the graph
(graph_node::update_connections on the device, D21), or the caller's upload.  What stays on the host: map_db_->set_local_landmarks, and the writes
to the landmark objects around the search (is_observable_in_tracking_, increase_num_observable).

Tables are torch tensors on the step's device, named as landmark_refresh_step names them where it has them:
  key frames  kf_erased [F] u8, kf_covis [F, 10] i32 (get_top_n_covisibilities(10), -1 padded), kf_parent [F] i32, kf_children_offsets [F + 1] i32,
              kf_children [C] i32, kf_lm [F, cap] i32 (keyfrm->get_landmarks() as rows, -1 = none; kf_landmarks_from_observations builds it where
              landmarks_ and observations_ agree), counts [F] or absent, kf_lm_lines [F, lcap] i32 with kl_counts [F], or absent = no lines
  landmarks   points: pos_w [L, 3] f64, normal [L, 3] f64, min_dist / max_dist [L] f32, desc [L, 32] u8, skip [L] u8 or absent (will_be_erased()),
              obs_offsets [L + 1] i32, obs_kf [T] i32; lines: pos_w_lines [LL, 6], min_dist_lines, max_dist_lines, desc_lines, skip_lines,
              obs_offsets_lines [LL + 1], and plucker_lines [LL, 6] where the caller keeps it
  frame       frm_lm [B, fcap] i32 (curr_frm_.landmarks_ as rows, -1 = none) with frm_counts [B] or absent, frm_lm_lines [B, flcap] with frm_kl_counts
              or absent, ref_kf [B] i32 or absent: the frames' ref_keyfrm_ before the call
"""


class local_map_step:
    def __init__(self, plp, k_cap=96, m_cap=4096, ml_cap=1024, max_num_local_keyfrms=60, workspace_bytes=0, device_index=0, mt=None):
        """k_cap, m_cap, ml_cap: rows per frame of the local key-frame, landmark and line lists (a longer list is a per-frame overflow status, D18;
        the second-order walk adds at most three key frames per first one, so 3 + max_num_local_keyfrms bounds the key frames unless more than
        max_num_local_keyfrms share a landmark with the frame)"""
        import torch
        self.torch, self.plp = torch, plp
        self.dev = torch.device("cuda", device_index)
        self.k_cap, self.m_cap, self.ml_cap = int(k_cap), int(m_cap), int(ml_cap)
        self.max_num_local_keyfrms, self.workspace_bytes = int(max_num_local_keyfrms), int(workspace_bytes)
        self.mt = mt or plp.matcher(device=device_index)

    def run(self, keyframes, landmarks, frame_landmarks, stream=None):
        """Enqueue both steps on `stream` (default: the current stream).  Returns dict(local: the dict run_local reads -- pos_w, normal, min_dist,
        max_dist, desc, counts, has_obs, skip and the _lines keys, rows behind a frame's count zero-filled from row 0 of the tables; ref_kf [B]; and the
        outputs of plp_local_map_device named as in LOCAL_MAP_OUTPUTS).  A frame whose status is LOCAL_MAP_NO_KEYFRAMES or LOCAL_MAP_KF_OVERFLOW has
        counts of 0: the tracker keeps its previous local map for the first.  Nothing is synchronised."""
        torch, plp = self.torch, self.plp
        st = stream or torch.cuda.current_stream(self.dev)
        i32, i64, u8 = torch.int32, torch.int64, torch.uint8
        frm = frame_landmarks["frm_lm"]
        B, fcap, F = frm.shape[0], frm.shape[1], keyframes["kf_parent"].shape[0]
        L, T = landmarks["pos_w"].shape[0], landmarks["obs_kf"].shape[0]
        lines = keyframes.get("kf_lm_lines") is not None
        LL = landmarks["pos_w_lines"].shape[0] if lines else 0
        frm_l = frame_landmarks.get("frm_lm_lines") if lines else None
        dims = dict(B=B, F=F, C=keyframes["kf_children"].shape[0], L=L, LL=LL, T=T, cap=keyframes["kf_lm"].shape[1],
                    lcap=keyframes["kf_lm_lines"].shape[1] if lines else 0, fcap=fcap, flcap=frm_l.shape[1] if frm_l is not None else 0,
                    k_cap=self.k_cap, m_cap=self.m_cap, ml_cap=self.ml_cap)
        tables = dict(kf_erased=keyframes.get("kf_erased"), kf_covis=keyframes["kf_covis"], kf_parent=keyframes["kf_parent"],
                      kf_children_offsets=keyframes["kf_children_offsets"], kf_children=keyframes["kf_children"], kf_lm=keyframes["kf_lm"],
                      kf_counts=keyframes.get("counts"), kf_lm_lines=keyframes.get("kf_lm_lines"), kf_kl_counts=keyframes.get("kl_counts") if lines else None,
                      obs_offsets=landmarks["obs_offsets"], obs_kf=landmarks["obs_kf"], lm_erased=landmarks.get("skip"),
                      lm_erased_lines=landmarks.get("skip_lines") if lines else None, frm_lm=frm, frm_counts=frame_landmarks.get("frm_counts"),
                      frm_lm_lines=frm_l, frm_kl_counts=frame_landmarks.get("frm_kl_counts") if frm_l is not None else None)
        for k, v in tables.items():
            if v is not None and not v.is_contiguous():
                raise plp.PlpError(plp.PLP_ERR_INVALID_ARG, f"{k} must be contiguous")
        tt = {"uint8": u8, "int32": i32}
        caps = dict(k_cap=self.k_cap, m_cap=self.m_cap, ml_cap=self.ml_cap)
        with torch.cuda.stream(st):
            out = {k: torch.zeros((B,) if c is None else (B, caps[c]), dtype=tt[dt.__name__], device=self.dev)
                   for k, (c, dt, _, line_side) in plp.LOCAL_MAP_OUTPUTS.items() if lines or not line_side}
        self.mt.local_map_device(dims, tables, {k: v for k, v in out.items() if v.numel()}, max_num_local_keyfrms=self.max_num_local_keyfrms,
                                 workspace_bytes=self.workspace_bytes, stream=st)
        with torch.cuda.stream(st):
            local = self._gather(landmarks, out["local_lm"], out["num_lm"], out["held"], "", L, self.m_cap)
            if lines:
                local.update(self._gather(landmarks, out["local_lines"], out["num_lines"], out["held_lines"], "_lines", LL, self.ml_cap))
            prev = frame_landmarks.get("ref_kf")
            prev = torch.full((B,), -1, dtype=i32, device=self.dev) if prev is None else prev.to(i32)
            keep = (out["nearest_kf"] < 0) | (out["status"] == plp.LOCAL_MAP_NO_KEYFRAMES)
            ref_kf = torch.where(keep, prev, out["nearest_kf"])
        return dict(out, local=local, ref_kf=ref_kf)

    def _gather(self, landmarks, rows, num, held, sfx, L, cap):
        """the rows of the landmark tables a list names, [B, cap, ...]; slots behind a frame's count read row 0 and are masked by counts"""
        torch = self.torch
        B = rows.shape[0]
        counts = num.clamp(0, cap).to(torch.int32)
        names = ["pos_w", "min_dist", "max_dist", "desc"] + ([] if sfx else ["normal"]) + (["plucker"] if sfx and "plucker_lines" in landmarks else [])
        res = {"counts" + sfx: counts}
        if L == 0 or cap == 0:
            for k in names:
                t = landmarks[k + sfx]
                res[k + sfx] = torch.zeros((B, cap) + tuple(t.shape[1:]), dtype=t.dtype, device=self.dev)
            res["has_obs" + sfx] = torch.zeros((B, cap), dtype=torch.uint8, device=self.dev)
            res["skip" + sfx] = torch.ones((B, cap), dtype=torch.uint8, device=self.dev)
            return res
        live = torch.arange(cap, device=self.dev)[None, :] < counts.to(torch.int64)[:, None]
        idx = torch.where(live, rows, torch.zeros_like(rows)).clamp(0, L - 1).to(torch.int64)
        for k in names:
            res[k + sfx] = landmarks[k + sfx][idx]
        off = landmarks["obs_offsets" + sfx].to(torch.int64)
        res["has_obs" + sfx] = (off[idx + 1] > off[idx]).to(torch.uint8)
        skip = held != 0
        if landmarks.get("skip" + sfx) is not None:
            skip = skip | (landmarks["skip" + sfx][idx] != 0)
        res["skip" + sfx] = (skip | ~live).to(torch.uint8)
        return res
