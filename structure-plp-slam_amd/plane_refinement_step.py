"""Plane refinement for one map on one stream, without the host: the map's plane table and landmark tables stay on the device, new planes from
`plane_step.run` are appended to the table and Planar_Mapping_module::refinement() (planar_mapping_module.cc:773-793: merge_planes,
refine_planes, refine_points) runs over it in place (plp_plane_refinement_device).

  planes      the map's plane table, `new_table()`: pl_state [NP_cap] u8 (PLANE_ROW_*), pl_equation [NP_cap, 4] f64, pl_best_error [NP_cap] f64,
              pl_count [NP_cap] i32, pl_lm [NP_cap, n_cap] i32 (landmark rows in slot order, -1 behind the count)
  landmarks   pos_w [L, 3] f64, lm_erased [L] u8, lm_owner [L] i32 (the row of get_Owning_Plane(), -1: none)

`append(planes, landmarks, created)` adds the P rows of a `plane_step.run` result at the next P rows of the table, at static shape: a PLANE_OK
row becomes IN_DB | VALID | NEED_REFINEMENT (a new data::Plane needs refinement, data/landmark_plane.cc:45; create_new_plane sets it valid) with
step [4]'s members in slot order as its list, its equation and best error as the fit left them; every other row gets state 0.  The owners
come from the result's lm_plane.  `run(planes, landmarks, dist_thresh, error_thresh)` enqueues the call and returns the views the rest of the
library reads -- equation, active (what plp_plane_refine_points_device calls active), lm_plane (= lm_owner) -- and the call's outputs; nothing is
synchronised.  `run_and_grow` is the form that reads the status back: a merge that would pass n_cap (PLANE_REFINEMENT_OVERFLOW) leaves the
tables undefined, so it keeps a copy, and on overflow restores it, doubles n_cap and runs again.

What stays on the host: new / delete of data::Plane, the colour copy of Plane::merge (from the outputs' merges), and
erase_landmark_plane (from the outputs' removed)."""


class plane_refinement_step:
    def __init__(self, plp, NP_cap, n_cap, points_per_ransac=18, iters=50, dot_product_threshold=0.8, offset_delta_factor=6, seed=0, merge_cap=16,
                 device_index=0):
        import torch
        self.torch, self.plp = torch, plp
        self.dev = torch.device("cuda", device_index)
        self.NP_cap, self.n_cap, self.ppr, self.iters = int(NP_cap), int(n_cap), int(points_per_ransac), int(iters)
        self.dot_thr, self.factor, self.seed, self.merge_cap = float(dot_product_threshold), int(offset_delta_factor), seed, int(merge_cap)
        if self.NP_cap > plp.PLANE_REFINEMENT_MAX_ROWS or self.n_cap > 8192:
            raise plp.PlpError(plp.PLP_ERR_UNSUPPORTED, "more than 4096 plane rows or 8192 slots per plane")
        self.mt = plp.matcher(device=device_index)
        self.next_row = 0

    def new_table(self):
        torch = self.torch
        z = lambda shape, dt, fill=0: torch.full(shape, fill, dtype=dt, device=self.dev)
        return dict(pl_state=z((self.NP_cap,), torch.uint8), pl_equation=z((self.NP_cap, 4), torch.float64), pl_best_error=z((self.NP_cap,), torch.float64),
                    pl_count=z((self.NP_cap,), torch.int32), pl_lm=z((self.NP_cap, self.n_cap), torch.int32, -1))

    def append(self, planes, landmarks, created, stream=None):
        """the rows of a plane_step.run result (for landmark tables of the same L) become rows next_row .. next_row + P - 1; returns the first row"""
        torch, plp = self.torch, self.plp
        P, cap = created["inliers"].shape
        row0 = self.next_row
        if row0 + P > self.NP_cap or cap > self.n_cap:
            raise plp.PlpError(plp.PLP_ERR_CAPACITY, "the plane table has no room for these rows")
        with torch.cuda.stream(stream or torch.cuda.current_stream(self.dev)):
            ok = created["status"] == plp.PLANE_OK
            member = (created["inliers"] == 1) & (created["slot_lm"] >= 0) & ok.unsqueeze(1)
            order = torch.sort((~member).to(torch.int8), dim=1, stable=True).indices               # the members first, in slot order
            count = member.sum(1).to(torch.int32)
            lst = torch.gather(created["slot_lm"], 1, order)
            lst = torch.where(torch.arange(cap, device=self.dev).unsqueeze(0) < count.unsqueeze(1), lst, torch.full_like(lst, -1))
            rows = slice(row0, row0 + P)
            planes["pl_state"][rows] = torch.where(ok, plp.PLANE_ROW_IN_DB | plp.PLANE_ROW_VALID | plp.PLANE_ROW_NEED_REFINEMENT, 0).to(torch.uint8)
            planes["pl_equation"][rows] = created["equation"]
            planes["pl_best_error"][rows] = created["best_error"]
            planes["pl_count"][rows] = count
            planes["pl_lm"][rows] = -1
            planes["pl_lm"][rows, :cap] = lst
            lp = created["lm_plane"]
            landmarks["lm_owner"].copy_(torch.where(lp >= 0, lp + row0, landmarks["lm_owner"]))
        self.next_row = row0 + P
        return row0

    def run(self, planes, landmarks, dist_thresh, error_thresh, stages=None, stream=None):
        """Enqueue refinement() on `stream` (default: the current stream); the tables are updated in place.  dist_thresh / error_thresh: numbers
        or f64 tensors of one element.  Returns dict(equation, active, lm_plane, and the outputs of PLANE_REFINEMENT_OUTPUTS, each [1, ...])."""
        torch, plp = self.torch, self.plp
        st = stream or torch.cuda.current_stream(self.dev)
        L = int(landmarks["lm_owner"].shape[0])
        with torch.cuda.stream(st):
            thr = lambda v: (v if torch.is_tensor(v) else torch.full((1,), float(v), dtype=torch.float64, device=self.dev)).to(torch.float64).reshape(1).contiguous()
            d_thr, e_thr = thr(dist_thresh), thr(error_thresh)
            out = {k: torch.zeros((1,) + shape(self.NP_cap, L, self.merge_cap), dtype=getattr(torch, dt.__name__), device=self.dev)
                   for k, (shape, dt) in plp.PLANE_REFINEMENT_OUTPUTS.items()}
        tables = dict(planes, pos_w=landmarks["pos_w"], lm_erased=landmarks["lm_erased"], lm_owner=landmarks["lm_owner"])
        self.mt.plane_refinement_device(1, self.NP_cap, planes["pl_lm"].shape[1], L, tables, d_thr, e_thr, out, points_per_ransac=self.ppr, iters=self.iters,
                                        dot_product_threshold=self.dot_thr, offset_delta_factor=self.factor, seed=self.seed,
                                        stages=plp.PLANE_STAGE_ALL if stages is None else stages, merge_cap=self.merge_cap, stream=st)
        with torch.cuda.stream(st):
            s = planes["pl_state"]
            live = plp.PLANE_ROW_IN_DB | plp.PLANE_ROW_VALID
            active = (((s & (live | plp.PLANE_ROW_NEED_REFINEMENT)) == live) & (planes["pl_count"] >= self.ppr)).to(torch.uint8)
        res = dict(equation=planes["pl_equation"], active=active, lm_plane=landmarks["lm_owner"])
        res.update(out)
        return res

    def run_and_grow(self, planes, landmarks, dist_thresh, error_thresh, stream=None):
        """run() behind a copy of the tables, with one wait for the status: on PLANE_REFINEMENT_OVERFLOW the copy is restored, pl_lm gets twice
        the slots (planes["pl_lm"] is replaced) and the call runs again"""
        torch, plp = self.torch, self.plp
        st = stream or torch.cuda.current_stream(self.dev)
        while True:
            with torch.cuda.stream(st):
                keep = {k: v.clone() for k, v in planes.items()}
                keep_lm = {k: landmarks[k].clone() for k in ("pos_w", "lm_owner")}
            res = self.run(planes, landmarks, dist_thresh, error_thresh, stream=st)
            st.synchronize()
            if int(res["status"][0]) != plp.PLANE_REFINEMENT_OVERFLOW:
                return res
            if 2 * planes["pl_lm"].shape[1] > 8192:
                raise plp.PlpError(plp.PLP_ERR_CAPACITY, "a plane's list would pass 8192 slots")
            with torch.cuda.stream(st):
                for k, v in keep.items():
                    if k != "pl_lm":
                        planes[k].copy_(v)
                for k, v in keep_lm.items():
                    landmarks[k].copy_(v)
                planes["pl_lm"] = torch.cat([keep["pl_lm"], torch.full_like(keep["pl_lm"], -1)], dim=1)
