// TEST INFRASTRUCTURE ONLY (oracle/_ref/libplpref3.so, see ../../README.md).  Stand-in for the reference's data/landmark_line.h with the
// members module/local_map_cleaner.cc:133-199 touches.
#ifndef PLP_REF_SHADOW_MAP_LANDMARK_LINE_H
#define PLP_REF_SHADOW_MAP_LANDMARK_LINE_H

namespace PLPSLAM
{
    namespace data
    {
        class Line
        {
        public:
            // landmark_line.cc:178-182
            unsigned int num_observations() const { return _num_observations; }

            // landmark_line.cc:284-302: the flag; a line of these scenes has no observation to take out of a key frame
            void prepare_for_erasing() { _will_be_erased = true; }

            // landmark_line.cc:304-309
            bool will_be_erased() { return _will_be_erased; }

            // landmark_line.cc:449-453
            float get_observed_ratio() const { return static_cast<float>(_num_observed) / _num_observable; }

            unsigned int _first_keyfrm_id = 0;

            unsigned int _num_observations = 0;
            unsigned int _num_observable = 1;
            unsigned int _num_observed = 1;
            bool _will_be_erased = false;
        };

    } // namespace data
} // namespace PLPSLAM

#endif
