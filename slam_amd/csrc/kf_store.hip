// kf_store.hip -- how the keyframe store lets go of a cloud: slam_kf_remove_keyframe and slam_kf_replace_keyframe_dev.
// Ids are positions in the store's vector and are never reissued: a removed keyframe stays there as an empty entry marked
// `removed`, which kf_live (kf_common.hpp) refuses for every call that names an id.  No kernel of its own: the replacement
// is slam_kf_add_keyframe_dev's filter and index, moved into the old id's entry once they stand.
#include "kf_common.hpp"

extern "C" {

int slam_kf_remove_keyframe(slam_kf_t *s, int id)
{
    SLAM_REQUIRE(kf_live(s, id), SLAM_E_INVALID, "slam_kf_remove_keyframe: no keyframe %d", id);
    // hipFree waits for the device itself: no enqueued registration still reads the blocks when they go
    Keyframe gone = std::move(s->kfs[id]);
    s->kfs[id] = Keyframe();
    s->kfs[id].removed = true;
    return SLAM_OK; // `gone` frees the cloud, its index and its covariances here
}

int slam_kf_replace_keyframe_dev(slam_kf_t *s, int id, const float *d_xyz, int n, int stride, slam_stream_t stream)
{
    SLAM_REQUIRE(kf_live(s, id), SLAM_E_INVALID, "slam_kf_replace_keyframe_dev: no keyframe %d", id);
    int fresh = -1;
    SLAM_TRY(slam_kf_add_keyframe_dev(s, d_xyz, n, stride, &fresh, stream)); // refused: the old keyframe stays
    // the new entry holds no covariances: they are computed again on demand.  The parameters they fixed stay fixed.
    s->kfs[id] = std::move(s->kfs[fresh]); // frees the old blocks (waits for the device)
    s->kfs.pop_back();
    return SLAM_OK;
}

} // extern "C"
