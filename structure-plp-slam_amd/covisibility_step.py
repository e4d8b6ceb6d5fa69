"""The covisibility graph after a new key frame, a fusion or a culling: data::graph_node (data/graph_node.cc:36-285) on
the tables local_map_step, local_ba_step, map_culling_step and place_recognition_step share, on one stream, without the host.

  run     update_connections() of the key frames `owners`, as if one after another (mapping_module.cc:353, :654; global_optimization_module.cc:217):
          plp_covisibility_update_device updates the graph's tables in `keyframes` in place
  erase   erase_all_connections() of the key frames of a mask (keyframe.cc:914), e.g. map_culling_step's kf_removed: plp_covisibility_erase_device

Both return the views the other steps read, all of static shape (torch gathers and integer scatters on the stream):
  kf_covis             [F, 10] i32, -1 padded: get_top_n_covisibilities(10) of every key frame, for local_map_step and plp_bow_query (with n_covis [F])
  kf_children_offsets, kf_children   [F + 1], [F] i32: the spanning children of every key frame in ascending row (D18's order), derived from kf_parent
                       by a stable sort; the rows behind kf_children_offsets[F] are the key frames without a parent
  covis_rows, covis_offsets   [G, covis_cap] i32 and [G, 2] i32 = [0, n]: get_covisibilities() of each owner, a problem of
                       map_culling_step.run_keyframes (run only)
  kf_local             [G, F] u8: the owner and its covisibilities, local_ba_step's problem (run only)
  reject               [G, F] u8: get_connected_keyframes() and the owner itself, place_recognition_step's mask (run only)

No .item(), no copy to the host, no boolean-mask indexing.  An overflow of a row (status COVIS_OVERFLOW, touched 2) is the caller's to see: the
tables must be wide enough (plp.covisibility_graph regrows, with the host in the loop).  What stays on the host: recover_spanning_connections and
the loop edges.

Tables are torch tensors on the step's device:
  key frames  kf_lm [F, cap] i32, counts [F] i32 or absent, kf_id [F] i32 (id_, the bits of an unsigned), and the graph: kf_conn, kf_conn_w
              [F, conn_cap] i32, kf_n_conn [F] i32, kf_covis_all, kf_covis_w [F, covis_cap] i32, kf_n_covis [F] i32, kf_parent [F] i32,
              kf_parent_unset [F] u8 (plp.covisibility_state names the full ordered table kf_covis; here kf_covis is the [F, 10] view the other
              steps read, which run and erase store back into `keyframes` with the children lists)
  landmarks   skip [L] u8 or absent (will_be_erased()), obs_offsets [L + 1] i32, obs_kf [T] i32
"""


class covisibility_step:
    TOP = 10

    def __init__(self, plp, device_index=0, mt=None):
        import torch
        self.torch, self.plp = torch, plp
        self.dev = torch.device("cuda", device_index)
        self.mt = mt or plp.matcher(device=device_index)

    @staticmethod
    def empty_graph(plp, F, conn_cap, covis_cap, device):
        """the graph's tables of F key frames without a connection, under the names this step uses"""
        import torch
        st = {k: torch.from_numpy(v).to(device) for k, v in plp.covisibility_state(F, conn_cap, covis_cap).items()}
        st["kf_covis_all"] = st.pop("kf_covis")
        return st

    def _state(self, keyframes, names):
        st = {k: keyframes["kf_covis_all" if k == "kf_covis" else k] for k in names}
        for k, v in st.items():
            if not v.is_contiguous():
                raise self.plp.PlpError(self.plp.PLP_ERR_INVALID_ARG, f"{k} must be contiguous")
        return st

    def _views(self, keyframes):
        """what every key frame's row gives the other steps; stored into `keyframes`"""
        torch = self.torch
        i32, i64 = torch.int32, torch.int64
        full, n = keyframes["kf_covis_all"], keyframes["kf_n_covis"]
        F, vc = full.shape
        top = torch.full((F, self.TOP), -1, dtype=i32, device=self.dev)
        top[:, :min(vc, self.TOP)] = full[:, :self.TOP]
        parent = keyframes["kf_parent"].to(i64)
        key = torch.where((parent >= 0) & (parent < F), parent, torch.full_like(parent, F))
        children = torch.sort(key, stable=True).indices.to(i32)                 # the children of a parent in ascending row
        per = torch.zeros(F + 1, dtype=i64, device=self.dev).index_add_(0, key, torch.ones_like(key))
        offsets = torch.cat([torch.zeros(1, dtype=i64, device=self.dev), per[:F].cumsum(0)]).to(i32)
        v = dict(kf_covis=top, n_covis=n.clamp(0, min(vc, self.TOP)).to(i32), kf_children_offsets=offsets, kf_children=children)
        keyframes.update(kf_covis=top, kf_children_offsets=offsets, kf_children=children)
        return v

    def _mask(self, owners, rows, n):
        """[G, F] u8: 1 at the owner and at the first n[g] entries of rows[g], by an integer scatter-add (the same result in any order)"""
        torch = self.torch
        G, width = rows.shape
        F = n.shape[0]
        own = owners.to(torch.int64).clamp(0, max(F - 1, 0))
        live = torch.arange(width, device=self.dev)[None, :] < n[own].clamp(0, width).to(torch.int64)[:, None]
        idx = torch.where(live & (rows >= 0) & (rows < F), rows.to(torch.int64), own[:, None])
        hit = torch.zeros((G, F), dtype=torch.int32, device=self.dev)
        hit.scatter_add_(1, idx, torch.ones_like(idx, dtype=torch.int32))
        return (hit > 0).to(torch.uint8)

    def run(self, keyframes, landmarks, owners, stream=None):
        """owners [G] i32: the rows, in call order.  Returns dict(status, nearest, max_weight [G], touched [F], and the views above)."""
        torch, plp = self.torch, self.plp
        st = stream or torch.cuda.current_stream(self.dev)
        i32, u8 = torch.int32, torch.uint8
        state = self._state(keyframes, plp.COVISIBILITY_STATE)
        kf_lm = keyframes["kf_lm"]
        F, cap, G = kf_lm.shape[0], kf_lm.shape[1], owners.shape[0]
        L, T = landmarks["obs_offsets"].shape[0] - 1, landmarks["obs_kf"].shape[0]
        tables = dict(kf_lm=kf_lm, kf_counts=keyframes.get("counts"), obs_offsets=landmarks["obs_offsets"], obs_kf=landmarks["obs_kf"],
                      lm_erased=landmarks.get("skip"), kf_id=keyframes["kf_id"], owners=owners)
        for k, v in tables.items():
            if v is not None and not v.is_contiguous():
                raise plp.PlpError(plp.PLP_ERR_INVALID_ARG, f"{k} must be contiguous")
        with torch.cuda.stream(st):
            out = dict(status=torch.zeros(G, dtype=u8, device=self.dev), nearest=torch.full((G,), -1, dtype=i32, device=self.dev),
                       max_weight=torch.zeros(G, dtype=i32, device=self.dev), touched=torch.zeros(F, dtype=u8, device=self.dev))
        dims = dict(F=F, L=L, T=T, cap=cap, conn_cap=state["kf_conn"].shape[1], covis_cap=state["kf_covis"].shape[1], G=G)
        self.mt.covisibility_update_device(dims, dict(tables, **state), {k: v for k, v in out.items() if v.numel()}, stream=st)
        with torch.cuda.stream(st):
            out.update(self._views(keyframes))
            if F:
                own = owners.to(torch.int64).clamp(0, F - 1)
                rows, vc = state["kf_covis"][own], state["kf_covis"].shape[1]
                n = state["kf_n_covis"][own].clamp(0, vc)
                out.update(covis_rows=rows.contiguous(), covis_offsets=torch.stack([torch.zeros_like(n), n], 1).to(i32).contiguous(),
                           kf_local=self._mask(owners, rows, state["kf_n_covis"]), reject=self._mask(owners, state["kf_conn"][own], state["kf_n_conn"]))
        return out

    def erase(self, keyframes, mask, stream=None):
        """mask [F] u8: the key frames whose connections go.  Returns dict(status, touched [F], and the per-key-frame views above)."""
        torch, plp = self.torch, self.plp
        st = stream or torch.cuda.current_stream(self.dev)
        state = self._state(keyframes, plp.COVISIBILITY_ERASE_STATE)
        F = mask.shape[0]
        if not mask.is_contiguous() or mask.dtype != torch.uint8:
            raise plp.PlpError(plp.PLP_ERR_INVALID_ARG, "mask must be a contiguous u8 tensor")
        with torch.cuda.stream(st):
            out = dict(status=torch.zeros(F, dtype=torch.uint8, device=self.dev), touched=torch.zeros(F, dtype=torch.uint8, device=self.dev))
        dims = dict(F=F, conn_cap=state["kf_conn"].shape[1], covis_cap=state["kf_covis"].shape[1])
        self.mt.covisibility_erase_device(dims, dict(state, erased=mask), {k: v for k, v in out.items() if v.numel()}, stream=st)
        with torch.cuda.stream(st):
            out.update(self._views(keyframes))
        return out
