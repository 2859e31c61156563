// msl_match_handle.h -- the matcher handle, shared by msl_match.hip, msl_line_match.hip, msl_pose.hip, msl_plane.hip and msl_bow.hip (internal).
#pragma once

#include "msl_common.h"

// One matcher object = one ORBmatcher of the reference (src/ORBmatcher.cc:41): its own stream and its own scratch, used by one thread at a time;
// the device is re-bound at every entry like the other handles.  The line searches (= the tracker's LSDmatcher) and msl_pose_optimize run on it too.
struct msl_match {
    int device = 0;
    hipStream_t stream = nullptr; bool ownStream = true;
    msl::DevBuf in[14], items, cellStart, mode, cand, candCnt, out[3];   // staged inputs (host-memory calls), scratch, staged outputs
    msl::DevBuf da, db, dout;                                          // msl_match_descriptor_distance
    msl::DevBuf lin[14], trk, inView;                                  // msl_match_local_points: staged inputs, per-point scratch
    msl::DevBuf poseIn[16], poseOut[5];                                // msl_pose_optimize[_translation]: staged inputs (+ Rcw), in/out flags, outputs
    msl::DevBuf lineIn[11], lineQ, lineTrk, lineView, lineIo[2];       // the line searches: staged inputs, per-line queries / tracks / in-view, line_xyz / line_has
    msl::DevBuf planeIn[8], planeDis, planeOut[5];                     // msl_plane_associate: staged inputs, [frame][map plane][64] distances, outputs
    msl::DevBuf mfIn[13], mfOut[4];                                    // msl_manhattan_detect: staged inputs, Rcw (in/out) and outputs
    msl::DevBuf bowIn[2], bowOut[5], bowW;                             // msl_bow_transform: staged inputs, outputs, per-feature word weights
    msl::DevBuf bmIn[9], bmOut[2];                                     // msl_match_by_bow
    msl::DevBuf ldIn[6], ldOut[4];                                     // msl_match_lines_by_descriptor (line_xyz in/out)
    bool bowAttrSet = false;
    bool lineAttrSet = false;
    bool localAttrSet = false;
    bool attrSet = false;
};

namespace msl {

// The device-indexed convenience entry points share one lazily created handle per device, serialised by one mutex.  The handles are
// never destroyed (see DevBuf).
extern msl_match *g_default[16];
extern std::mutex g_default_mutex;

inline msl_match *default_handle(int device) {   // g_default_mutex held
    msl_match *&h = g_default[device & 15];
    if (!h) h = msl_match_create(device);
    return h;
}

// A *_batch form: run(h) on the device's shared handle, synchronous.  sync_legacy: the call reads device memory that is complete, or
// enqueued on the legacy default stream, when the call is made (as before the handle existed).
template <class Run>
int on_default_handle(int device, bool sync_legacy, Run run) {
    std::lock_guard<std::mutex> lock(g_default_mutex);
    msl_match *h = default_handle(device);
    if (!h) return MSL_ERR_NO_DEVICE;
    if (sync_legacy) { if (bind_device(device) == MSL_OK) (void)hipStreamSynchronize(0); }
    int rc = run(h);
    if (rc == MSL_OK) rc = msl_match_sync(h);
    return rc;
}

}  // namespace msl
