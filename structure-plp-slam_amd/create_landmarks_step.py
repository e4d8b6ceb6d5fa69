"""The point half of the mapping thread's landmark creation for G current key frames at once: poses and feature tables in, the key-point
pairs and positions of the new landmarks and the updated occupancy out, on one stream, without the host.

For G current key frames with N neighbours each, `create_landmarks_step.run` does what mapping_module::create_new_landmarks
(mapping_module.cc:359-479) does per neighbour with triangulate_with_two_keyframes (:420-479):

  once       plp_median_depth_device                   keyframe::compute_median_depth(true) of every key frame (monocular gate)
  once       plp_keyframe_pair_geometry_device         the baseline gate, E_12 and the epipole of all G x N pairs
  per rank   PLP_MATCH_MODE_TRIANGULATION              robust::match_for_triangulation(cur, ngh, E_12), epipolar built on the device
             plp_triangulate_keypoint_pairs_device     two_view_triangulator::triangulate of every match, occupied_*_io updated in place

The ranks run one after the other: neighbour i + 1's matcher must skip the key points that got a landmark with neighbour i
(keyframe::add_landmark, :464-465), so its q_valid is gathered from the running occupancy of the current key frame.  The G key frames are
the batch: they are independent problems, each with its own copy of its neighbours' occupancy (a neighbour shared by two current key
frames of one batch does not see the other's landmarks, as it would not if the two were processed in two mapping threads).

The matcher's queries are the current key frame's key points in BoW node order (ascending node, ascending index inside a node -- the order
robust.cc:73-108 walks the feature vector in); the step derives that order from the node ids with a stable sort and passes it on as
q_feature.  Gathering the query arrays is torch indexing on the stream; the geometry, the search and the triangulation are the library's
kernels.

What stays on the host: `new data::landmark`, add_observation, map_db_->add_landmark and local_map_cleaner_->add_fresh_landmark (:459-477),
which build map objects from the (idx_1, idx_2, pos_w) triples the step returns (compute_descriptor and update_normal_and_depth of the new
landmarks: landmark_refresh_step.py); and the
`1 < i && keyframe_is_queued()` abort (:374), which a caller honours by passing fewer neighbours.

Tables are torch tensors on the step's device, F key frames of `cap` key-point slots:
  kps [F, cap, 28] u8 (undist_keypts_ as plp_keypoint), desc [F, cap, 32] u8, node [F, cap] i32 (the BoW node of every key point),
  bearings [F, cap, 3] f64, counts [F] i32, occupied [F, cap] u8 (key point has a landmark), pose [F, 15] f64 (frame_pose rows),
  x_right / depths [F, cap] f32 (stereo, RGB-D), lm_pos_w [F, m, 3] f64 / lm_valid [F, m] u8 (the key frames' landmarks: monocular gate)
"""
import numpy as np


class create_landmarks_step:
    def __init__(self, plp, camera, setup_type=0, true_baseline=0.0, scale_factor=1.2, num_levels=8, rays_parallax_deg_thr=1.0, device_index=0):
        """camera: a plp.camera_model_c.  The matcher is match::robust(0.0, false) as mapping_module.cc:425 constructs it."""
        import torch
        self.torch, self.plp, self.camera = torch, plp, camera
        self.dev = torch.device("cuda", device_index)
        self.setup_type, self.true_baseline = int(setup_type), float(true_baseline)
        self.scale_factor, self.thr = float(scale_factor), float(rays_parallax_deg_thr)
        sf = np.ones(num_levels, np.float32)
        for i in range(1, num_levels):                          # orb_params::calc_scale_factors / calc_level_sigma_sq: float products
            sf[i] = np.float32(sf[i - 1] * np.float32(scale_factor))
        self.sf, self.sigma_sq = sf, (sf * sf).astype(np.float32)
        self.mt = plp.matcher(lowe_ratio=0.0, check_orientation=False, device=device_index)

    def run(self, table, cur, neighbours, stream=None):
        """cur [G] and neighbours [G, N] (int64 tensors): indices into the table; every entry names a key frame.  Enqueues everything on
        `stream` (default: the current stream) and returns, without synchronising, dict(idx_1 [N, G, cap] i32, pos_w [N, G, cap, 3] f64,
        status [N, G, cap] u8: per rank, current key frame and key point t of the neighbour (plp_keypoint_pair_status; a landmark where
        status == 0: key points idx_1 of cur and t of the neighbour at pos_w), skip [N, G] u8, epipolar [N, G, 12], baseline [N, G],
        num_matches [N, G] i32, occupied_cur [G, cap] u8: cur's occupancy after all ranks, occupied_ngh [N, G, cap] u8: the neighbours')."""
        torch, plp = self.torch, self.plp
        st = stream or torch.cuda.current_stream(self.dev)
        i32, f32, f64, u8, i64 = torch.int32, torch.float32, torch.float64, torch.uint8, torch.int64
        F, cap = table["kps"].shape[0], table["kps"].shape[1]
        G, N = neighbours.shape
        mono = self.setup_type == 0
        with torch.cuda.stream(st):
            new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.dev)
            out = dict(idx_1=torch.full((N, G, cap), -1, dtype=i32, device=self.dev), pos_w=new((N, G, cap, 3), f64), status=new((N, G, cap), u8),
                       skip=new((N, G), u8), epipolar=new((N, G, 12), f64), baseline=new((N, G), f64), num_matches=new((N, G), i32))
            if G == 0 or N == 0 or cap == 0:
                out.update(occupied_cur=table["occupied"][cur].clone(), occupied_ngh=new((N, G, cap), u8))
                return out
            pairs = torch.stack([cur.view(1, G).expand(N, G), neighbours.t()], 2).to(i32).contiguous()      # [N, G, 2], rank-major
            median = None
            if mono:
                median, count = new((F,), f32), new((F,), i32)
                m = table["lm_pos_w"].shape[1]
                self.mt.median_depth_device(F, m, table["pose"], table["lm_pos_w"], median, count, valid=table.get("lm_valid"), stream=st)
            self.mt.keyframe_pair_geometry_device(self.camera, self.setup_type, F, N * G, table["pose"], pairs, out["skip"], out["epipolar"],
                                                  out["baseline"], median_depth=median, true_baseline=self.true_baseline, stream=st)
            # the features as the matcher reads them: angle and octave out of the key-point records
            angle = table["kps"].view(f32)[:, :, 3].contiguous()
            octave = table["kps"].view(i32)[:, :, 5].contiguous()
            counts = table["counts"].to(i32)
            slot = torch.arange(cap, device=self.dev).view(1, cap)
            live = slot < counts.view(F, 1)
            # BoW node order of every key frame's key points: ascending node, ascending index inside a node; the slots past the count last
            key = torch.where(live, table["node"].to(i64), torch.full((), 1 << 40, dtype=i64, device=self.dev))
            order = torch.sort(key, dim=1, stable=True)[1]                                                   # [F, cap] query slot -> key point
            c_order = order[cur]                                                                             # [G, cap]
            q_feature = c_order.to(i32).contiguous()
            take = lambda a: torch.gather(a[cur], 1, c_order if a.dim() == 2 else c_order.view(G, cap, 1).expand(G, cap, a.shape[2])).contiguous()
            q = dict(q_desc=take(table["desc"]), q_angle=take(angle), q_group=take(table["node"].to(i32)), q_level=take(octave),
                     q_bearing=take(table["bearings"]), q_counts=counts[cur].contiguous())
            xr = table.get("x_right")
            if xr is not None and not mono:
                q["q_x_right"] = take(xr)
            occ_cur = table["occupied"][cur].clone()                                                         # [G, cap], running
            occ_ngh = new((N, G, cap), u8)
            for i in range(N):
                ngh = neighbours[:, i]
                occ_ngh[i].copy_(table["occupied"][ngh])
                t = dict(t_desc=table["desc"][ngh].contiguous(), t_angle=angle[ngh].contiguous(), t_group=table["node"][ngh].to(i32).contiguous(),
                         t_occupied=occ_ngh[i], t_bearing=table["bearings"][ngh].contiguous(), t_counts=counts[ngh].contiguous())
                if xr is not None and not mono:
                    t["t_x_right"] = xr[ngh].contiguous()
                q_valid = (1 - torch.gather(occ_cur, 1, c_order).clamp(max=1)).to(u8).contiguous()          # "has no landmark", in query order
                match_q = torch.full((G, cap), -1, dtype=i32, device=self.dev)
                self.mt.match_device(plp.MODE_TRIANGULATION, cap, cap, dict(q_valid=q_valid, epipolar=out["epipolar"][i], **q, **t), match_q,
                                     out["num_matches"][i], scale_factors=self.sf, B=G, stream=st)
                out["num_matches"][i].mul_(1 - out["skip"][i].to(i32))                                       # a gated pair never reaches the matcher
                self.mt.triangulate_keypoint_pairs_device(
                    self.camera, self.setup_type, F, cap, cap, G, table["kps"], table["bearings"], table["pose"], pairs[i], match_q, out["idx_1"][i],
                    out["pos_w"][i], out["status"][i], self.sf, self.sigma_sq, x_right=None if mono else xr, depths=None if mono else table.get("depths"),
                    counts=counts, q_feature=q_feature, pair_skip=out["skip"][i], occupied_1_io=occ_cur, occupied_2_io=occ_ngh[i],
                    true_baseline=self.true_baseline, scale_factor=self.scale_factor, rays_parallax_deg_thr=self.thr, stream=st)
            out.update(occupied_cur=occ_cur, occupied_ngh=occ_ngh, q_feature=q_feature)
        return out
