// TEST INFRASTRUCTURE ONLY (oracle/_ref/libplpref3.so, see ../../README.md).  Stand-in for the reference's data/landmark.h with the members
// data/graph_node.cc and module/local_map_cleaner.cc touch.  landmark.cc and keyframe.cc need Eigen and the map database and are not compiled;
// the cascade an erased key frame sets off is restated here from their text, line by line, with the lines cited.  That cascade is a second
// restatement, independent of tests/map_cull_ref.py; it is not a pin.
#ifndef PLP_REF_SHADOW_MAP_LANDMARK_H
#define PLP_REF_SHADOW_MAP_LANDMARK_H

#include <map>

#include "PLPSLAM/data/keyframe.h"

namespace PLPSLAM
{
    namespace data
    {
        class Plane;

        class landmark
        {
        public:
            // landmark.cc:80-97
            void add_observation(keyframe *keyfrm, unsigned int idx)
            {
                if (observations_.count(keyfrm))
                {
                    return;
                }
                observations_[keyfrm] = idx;

                if (0 <= keyfrm->stereo_x_right_.at(idx))
                {
                    num_observations_ += 2;
                }
                else
                {
                    num_observations_ += 1;
                }
            }

            // landmark.cc:99-136 (ref_keyfrm_, :119-122, is read by nothing compiled here and is left out)
            void erase_observation(keyframe *keyfrm)
            {
                bool discard = false;
                {
                    if (observations_.count(keyfrm))
                    {
                        int idx = observations_.at(keyfrm);
                        if (0 <= keyfrm->stereo_x_right_.at(idx))
                        {
                            num_observations_ -= 2;
                        }
                        else
                        {
                            num_observations_ -= 1;
                        }

                        observations_.erase(keyfrm);

                        // :124-128
                        if (num_observations_ <= 2)
                        {
                            discard = true;
                        }
                    }
                }

                if (discard)
                {
                    prepare_for_erasing();
                }
            }

            // landmark.cc:138-142
            std::map<keyframe *, unsigned int> get_observations() const { return observations_; }

            // landmark.cc:144-148
            unsigned int num_observations() const { return num_observations_; }

            // landmark.cc:365-383 (map_db_->erase_landmark, :382, has no map database to act on)
            void prepare_for_erasing()
            {
                std::map<keyframe *, unsigned int> observations;

                {
                    observations = observations_;
                    observations_.clear();
                    will_be_erased_ = true;
                }

                for (const auto &keyfrm_and_idx : observations)
                {
                    keyfrm_and_idx.first->erase_landmark_with_index(keyfrm_and_idx.second);
                }
            }

            // landmark.cc:385-390
            bool will_be_erased() { return will_be_erased_; }

            // landmark.cc:453-457
            float get_observed_ratio() const { return static_cast<float>(num_observed_) / num_observable_; }

            // landmark.cc:468-472
            Plane *get_Owning_Plane() const { return _mOwningPlane; }

            unsigned int first_keyfrm_id_ = 0;

            std::map<keyframe *, unsigned int> observations_;
            unsigned int num_observations_ = 0;
            unsigned int num_observable_ = 1;
            unsigned int num_observed_ = 1;
            bool will_be_erased_ = false;
            Plane *_mOwningPlane = nullptr;
        };

        // keyframe.cc:872-926.  Steps 3 and 4 past erase_all_connections() (recover_spanning_connections, the map and BoW databases) act on
        // objects no loop of local_map_cleaner.cc reads and are left out; _landmarks_line (:902-909) is empty here.
        inline void keyframe::prepare_for_erasing()
        {
            // :874-878
            if (origin_keyfrm_ && *this == *origin_keyfrm_)
            {
                return;
            }

            // :880-884
            if (cannot_be_erased_)
            {
                return;
            }

            // :888
            will_be_erased_ = true;

            // :892-899
            for (const auto lm : landmarks_)
            {
                if (!lm)
                {
                    continue;
                }
                lm->erase_observation(this);
            }

            // :914, the reference's own graph_node
            graph_node_->erase_all_connections();
        }

    } // namespace data
} // namespace PLPSLAM

#endif
