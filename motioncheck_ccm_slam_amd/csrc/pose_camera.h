// pose_camera.h -- a keyframe's Tcw / Ow (what ccm_frame_set_pose stores) from an optimised SE3Quat, as one definition for the host
// (ccm_pose_to_camera, and the handle's host copy after ccm_ba_solve_table_frames) and for k_ba_publish_table (ba_table.hip):
//   Tcw   Converter::toCvMat(SE3Quat) (Converter.cc:86-93): the quaternion's rotation matrix and the translation, each narrowed to
//         float -- rows 0-2 of what ccm_pose_to_mat4f gives
//   Ow    -Rwc * tcw as KeyFrame::SetPose evaluates it on the float matrices (src/KeyFrame.cpp:299-302), in the reading
//         Tracking.camera (tracking.py) states: the float entries widened, the three products summed left to right in double,
//         narrowed once.
// Every operation is one IEEE operation in the order written; the library is built with -ffp-contract=off, so the host and the
// device compiler give the same bits.
#pragma once
#include "ba_math.h"

BA_HD void ba_pose_to_camera(const double* pose7, float* Tcw, float* Ow)
{
    double R[9];
    ba_quat_to_R(pose7, R);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Tcw[i * 4 + j] = (float)R[i * 3 + j];
        Tcw[i * 4 + 3] = (float)pose7[4 + i];
    }
    const double t0 = (double)Tcw[3], t1 = (double)Tcw[7], t2 = (double)Tcw[11];
    for (int r = 0; r < 3; r++)
        Ow[r] = (float)(((-(double)Tcw[r]) * t0 - (double)Tcw[4 + r] * t1) - (double)Tcw[8 + r] * t2);
}
