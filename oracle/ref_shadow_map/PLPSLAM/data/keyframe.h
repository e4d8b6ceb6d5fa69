// TEST INFRASTRUCTURE ONLY (oracle/_ref/libplpref3.so, see ../../README.md).  Stand-in for the reference's data/keyframe.h with the members
// data/graph_node.cc and module/local_map_cleaner.cc touch and nothing else.  graph_node_ is the REFERENCE'S OWN class (its header is read from
// the reference tree, its code is graph_node.cc compiled unmodified); what this file restates from keyframe.{h,cc} is marked with the lines it
// restates.  Nothing restated here is a pin: see the README for what the reference's object code supplies and what these stand-ins do.
#ifndef PLP_REF_SHADOW_MAP_KEYFRAME_H
#define PLP_REF_SHADOW_MAP_KEYFRAME_H

#include <algorithm>
#include <atomic>
#include <cassert>
#include <functional>
#include <memory>
#include <vector>

#include "PLPSLAM/data/graph_node.h"

namespace PLPSLAM
{
    namespace data
    {
        class landmark;

        struct keypoint_stand_in // cv::KeyPoint: only .octave is read (local_map_cleaner.cc:280, :298)
        {
            int octave = 0;
        };

        class keyframe
        {
        public:
            keyframe() : graph_node_(new graph_node(this)) {}

            // keyframe.h:77
            bool operator==(const keyframe &keyfrm) const { return id_ == keyfrm.id_; }

            // keyframe.cc: a copy of landmarks_
            std::vector<landmark *> get_landmarks() const { return landmarks_; }

            // keyframe.cc:372-376
            void erase_landmark_with_index(const unsigned int idx) { landmarks_.at(idx) = nullptr; }

            // keyframe.cc:861
            void set_not_to_be_erased() { cannot_be_erased_ = true; }

            // keyframe.cc:872-926, defined in landmark.h (it needs landmark::erase_observation)
            void prepare_for_erasing();

            // keyframe.cc:928-931
            bool will_be_erased() { return will_be_erased_; }

            unsigned int id_ = 0;
            float depth_thr_ = 0.0f;
            std::vector<keypoint_stand_in> undist_keypts_;
            std::vector<float> stereo_x_right_;
            std::vector<float> depths_;
            const std::unique_ptr<graph_node> graph_node_;

            std::vector<landmark *> landmarks_;
            //! map_db_->origin_keyfrm_ (keyframe.cc:875); nullptr when no key frame of the scene carries the origin's id
            keyframe *origin_keyfrm_ = nullptr;
            std::atomic<bool> cannot_be_erased_{false};
            std::atomic<bool> will_be_erased_{false};
        };

    } // namespace data
} // namespace PLPSLAM

#endif
