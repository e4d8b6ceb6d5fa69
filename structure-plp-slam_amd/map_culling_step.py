"""Map culling after a new key frame: the two map-only calls of the mapping loop, module::local_map_cleaner (module/local_map_cleaner.cc:51-320;
DESIGN.md section 5, D20), on the tables local_ba_step, local_map_step and landmark_refresh_step share, on one stream, without the host.

  run_landmarks   remove_redundant_landmarks[_line] (mapping_module.cc:215-221): plp_cull_landmarks_device, then -- for one list -- the ERASE
                  states ORed into the landmark `skip` table in place
  run_keyframes   remove_redundant_keyframes (mapping_module.cc:284): plp_cull_keyframes_device, then -- for one problem -- out_kf_removed ORed
                  into `kf_erased` and out_lm_erased into `skip` in place: the tables the next local_map_step or landmark_refresh_step call reads

Several lists or problems are independent readings of one snapshot: their masks are returned and nothing is written back.  No .item(), no copy
to the host, no boolean-mask indexing.  erase_all_connections of the removed key frames is covisibility_step.erase over kf_removed (D21), and the
covisibility list of a problem is that step's view of the owner's row.  What stays on the host is the rest of what prepare_for_erasing() does to
objects: recover_spanning_connections, replace_reference_keyframe and the databases, for the rows the decisions name, in list order.

Tables are torch tensors on the step's device, named as the other steps name them:
  key frames  kps [F, kp_stride, 28] u8 (undist_keypts_ as plp_keypoint), counts [F] i32 or absent, kf_lm [F, cap] i32, kf_erased [F] u8 (updated in
              place), x_right [F, kp_stride] f32 (absent = monocular weights), and for this step kf_id [F] i32 (id_, the bits of an unsigned),
              kf_cannot_erase [F] u8 or absent, depths [F, kp_stride] f32 and depth_thr [F] f32 unless the cleaner is monocular
  landmarks   skip [L] u8 (will_be_erased(); updated in place), obs_offsets [L + 1] i32, obs_kf / obs_idx [T] i32, num_obs [L] i32 or absent
              (num_observations_; absent = derived from the lists), and for run_landmarks num_observed, num_observable, first_kf_id [L] i32 and
              owning_plane [L] u8 or absent; the line tables carry the suffix _lines
"""


class map_culling_step:
    def __init__(self, plp, is_monocular, origin_keyfrm_id=0, device_index=0, mt=None):
        import torch
        self.torch, self.plp, self.is_monocular, self.origin_keyfrm_id = torch, plp, bool(is_monocular), int(origin_keyfrm_id)
        self.dev = torch.device("cuda", device_index)
        self.mt = mt or plp.matcher(device=device_index)

    def _rows(self, v, n):
        """an int or a tensor as n i32 on the device"""
        torch = self.torch
        if torch.is_tensor(v):
            return v.reshape(-1).to(torch.int32).contiguous()
        return torch.full((n,), int(v), dtype=torch.int32, device=self.dev)

    def run_landmarks(self, landmarks, fresh, cur_kf_id, fresh_offsets=None, num_obs_thr=None, lines=False, stream=None):
        """fresh [N] i32: the fresh buffer as landmark rows -- one list, or R lists with fresh_offsets [R + 1]; cur_kf_id and num_obs_thr: an int
        or [R] (default: 2 or 3 by is_monocular for points, 3 for lines).  Returns dict(state [N], num_removed [R], num_fresh [R], fresh [N]: the
        lists afterwards, each inside its own run, -1 behind them).  One list: landmarks["skip" (+ "_lines")] takes the ERASE entries in place."""
        torch, plp = self.torch, self.plp
        st = stream or torch.cuda.current_stream(self.dev)
        sfx = "_lines" if lines else ""
        i32, u8 = torch.int32, torch.uint8
        N, L = fresh.shape[0], landmarks["num_observed" + sfx].shape[0]
        R = 1 if fresh_offsets is None else fresh_offsets.shape[0] - 1
        with torch.cuda.stream(st):
            off = torch.tensor([0, N], dtype=i32, device=self.dev) if fresh_offsets is None else fresh_offsets
            thr = self._rows(3 if lines or not self.is_monocular else 2, R) if num_obs_thr is None else self._rows(num_obs_thr, R)
            cur = self._rows(cur_kf_id, R)
            out = dict(state=torch.zeros(N, dtype=u8, device=self.dev), num_removed=torch.zeros(R, dtype=i32, device=self.dev),
                       num_fresh=torch.zeros(R, dtype=i32, device=self.dev), fresh=torch.full((N,), -1, dtype=i32, device=self.dev))
        skip = landmarks.get("skip" + sfx)
        tables = dict(fresh_offsets=off, fresh=fresh, lm_erased=skip, num_observed=landmarks["num_observed" + sfx],
                      num_observable=landmarks["num_observable" + sfx], first_kf_id=landmarks["first_kf_id" + sfx], num_obs=landmarks["num_obs" + sfx],
                      owning_plane=None if lines else landmarks.get("owning_plane"), cur_kf_id=cur, num_obs_thr=thr)
        for k, v in tables.items():
            if v is not None and not v.is_contiguous():
                raise plp.PlpError(plp.PLP_ERR_INVALID_ARG, f"{k} must be contiguous")
        if R and N:
            self.mt.cull_landmarks_device(dict(R=R, N=N, L=L), tables, out, stream=st)
        elif R:
            self.mt.cull_landmarks_device(dict(R=R, N=N, L=L), tables, {k: out[k] for k in ("num_removed", "num_fresh")}, stream=st)
        if R == 1 and N and L and skip is not None:
            with torch.cuda.stream(st):
                hit = torch.zeros(L, dtype=i32, device=self.dev)     # an integer scatter-add: the same result in any order
                hit.index_put_((fresh.to(torch.int64).clamp(0, L - 1),), (out["state"] == plp.CULL_ERASE).to(i32), accumulate=True)
                skip.bitwise_or_((hit > 0).to(u8))
        return out

    def run_keyframes(self, keyframes, landmarks, cur_kf, covis, covis_offsets=None, stream=None):
        """cur_kf: the row of the current key frame (an int, or [G] i32 with covis_offsets [G + 1]); covis [Cv] i32: the rows of its
        get_covisibilities(), in order.  Returns dict(num_removed [G], decision, num_valid, num_redundant [Cv], kf_removed [G, F], lm_erased
        [G, L]).  One problem: keyframes["kf_erased"] and landmarks["skip"] take the two masks in place."""
        torch, plp = self.torch, self.plp
        st = stream or torch.cuda.current_stream(self.dev)
        i32, u8 = torch.int32, torch.uint8
        kps, kf_lm = keyframes["kps"], keyframes["kf_lm"]
        F, cap, L, T, Cv = kf_lm.shape[0], kf_lm.shape[1], landmarks["obs_offsets"].shape[0] - 1, landmarks["obs_kf"].shape[0], covis.shape[0]
        G = 1 if covis_offsets is None else covis_offsets.shape[0] - 1
        with torch.cuda.stream(st):
            off = torch.tensor([0, Cv], dtype=i32, device=self.dev) if covis_offsets is None else covis_offsets
            cur = self._rows(cur_kf, G)
            out = dict(num_removed=torch.zeros(G, dtype=i32, device=self.dev), decision=torch.zeros(Cv, dtype=u8, device=self.dev),
                       num_valid=torch.zeros(Cv, dtype=i32, device=self.dev), num_redundant=torch.zeros(Cv, dtype=i32, device=self.dev),
                       kf_removed=torch.zeros((G, F), dtype=u8, device=self.dev), lm_erased=torch.zeros((G, L), dtype=u8, device=self.dev))
        tables = dict(kf_lm=kf_lm, kf_counts=keyframes.get("counts"), undist=kps, x_right=keyframes.get("x_right"), depths=keyframes.get("depths"),
                      depth_thr=keyframes.get("depth_thr"), kf_id=keyframes["kf_id"], kf_erased=keyframes.get("kf_erased"),
                      kf_cannot_erase=keyframes.get("kf_cannot_erase"), obs_offsets=landmarks["obs_offsets"], obs_kf=landmarks["obs_kf"],
                      obs_idx=landmarks["obs_idx"], lm_erased=landmarks.get("skip"), lm_num_obs=landmarks.get("num_obs"), cur_kf=cur, covis_offsets=off,
                      covis=covis)
        for k, v in tables.items():
            if v is not None and not v.is_contiguous():
                raise plp.PlpError(plp.PLP_ERR_INVALID_ARG, f"{k} must be contiguous")
        self.mt.cull_keyframes_device(dict(F=F, L=L, T=T, cap=cap, kp_stride=kps.shape[1], G=G, Cv=Cv), tables, {k: v for k, v in out.items() if v.numel()},
                                      origin_id=self.origin_keyfrm_id, is_monocular=self.is_monocular, stream=st)
        if G == 1:
            with torch.cuda.stream(st):
                if keyframes.get("kf_erased") is not None:
                    keyframes["kf_erased"].bitwise_or_(out["kf_removed"][0])
                if landmarks.get("skip") is not None:
                    landmarks["skip"].bitwise_or_(out["lm_erased"][0])
        return out
