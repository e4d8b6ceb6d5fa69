"""Loop-candidate search for Q key frames at once: descriptors in, candidate masks over the key-frame database out, on one stream, without the
host.

For Q query key frames whose descriptors are already in HBM, `place_recognition_step.run` does what loop_detector::detect_loop_candidates
(module/loop_detector.cc:66-93) does per key frame up to the point where it starts to work on keyframe objects:

  1  plp_bow_transform_device      keyframe::compute_bow (data/frame.cc:785-795)                    the queries' BowVectors
  2  plp_bow_score_pairs_device    the scores of compute_min_score_in_covisibilities (:238-266)     query q against each of its covisibilities
  3  torch, on the stream          min_score[q] = min(1.0f, the scores of the valid slots)          a [Q] device array; it never visits the host
  4  plp_bow_query_device          bow_database::acquire_loop_candidates (bow_database.cc:97-168)   final [Q, N] u8 and the per-row outputs

Step 3 is two torch operations of static shape (where, amin): no .item(), no copy to the host.  The score is DBoW2's L1 score restated from the
published algorithm: parity unpinned.

What stays on the host: the covisibility graph (the caller passes get_covisibilities() of every query as database rows, and a flag per slot
that is 0 for an unused slot or a key frame that will_be_erased()), the rejected key frames (get_connected_keyframes() and the query itself, as a
[Q, N] mask), and everything after the mask -- find_continuously_detected_keyframe_sets and the rest of the loop detector work on keyframe
objects -- as well as bow_database.add_keyframe of the queries afterwards (their BowVectors are in the returned tensors).

Tensors on the step's device:
  desc [Q, cap, 32] u8, counts [Q] i32 or None     the queries' descriptors (cap at most the database's stride)
  covis_rows [Q, C] i32, covis_valid [Q, C] u8     the queries' covisibilities as database rows; C >= 1
  reject [Q, N] u8 or None                          N = database.N
"""


class place_recognition_step:
    def __init__(self, plp, vocabulary, database, levelsup=4):
        """vocabulary: a plp.bow_vocabulary; database: a plp.bow_database on the same device"""
        import torch
        self.torch, self.plp, self.voc, self.db, self.levelsup = torch, plp, vocabulary, database, int(levelsup)
        self.dev = database.dev

    def run(self, desc, counts, covis_rows, covis_valid, reject=None, stream=None):
        """Enqueue the chain on `stream` (default: the current stream).  Returns dict(bow: the transform's tensors of the queries, pair_score
        [Q, C] f32, min_score [Q] f32, and the outputs of plp_bow_query_device: common, score, total, best_kf, final [Q, N]; n_final, max_common,
        best_total, status [Q]).  Nothing is synchronised."""
        torch, db = self.torch, self.db
        st = stream or torch.cuda.current_stream(self.dev)
        Q, cap = desc.shape[0], desc.shape[1]
        C = covis_rows.shape[1]
        with torch.cuda.stream(st):
            bow = self.voc.transform_device(desc, counts, self.levelsup, stream=st)
            a_row = torch.arange(Q, dtype=torch.int32, device=self.dev).repeat_interleave(C)
            b_row = covis_rows.reshape(-1).contiguous()
            pair = torch.empty((Q * C,), dtype=torch.float32, device=self.dev)
        t = db.t
        db.mt.bow_score_pairs_device(Q, cap, bow["bow_word"], bow["bow_value"], bow["n_bow"], db.N, db.stride, t["word"], t["value"], t["n"], Q * C, a_row,
                                     b_row, pair, scoring=db.scoring, stream=st)
        with torch.cuda.stream(st):
            pair = pair.reshape(Q, C)
            one = torch.ones((), dtype=torch.float32, device=self.dev)
            min_score = torch.where(covis_valid != 0, pair, one).amin(dim=1).clamp(max=1.0).contiguous()   # float min_score = 1.0; if (score < min_score) ...
        out = db.acquire_loop_candidates_device(bow["bow_word"], bow["bow_value"], bow["n_bow"], min_score, reject, stream=st)
        out.update(bow=bow, pair_score=pair, min_score=min_score)
        return out
