// ba_rig.h -- Tcam11 and Tcam21 as both bundle adjustments of the reference build them from the rig (src/Optimizer.cc:122-136 and
// :1048-1061: the same statements on mRcam12 / mtcam12 or on the rows of CalibMatrix), in cv::Mat float arithmetic, into the two 4x4
// row-major matrices of orbm_lba_problem::Tcim.  ONE definition for host/LocalBA.cc and host/GlobalBA.cc.
#ifndef MORB_BA_RIG_H
#define MORB_BA_RIG_H

#include "cv_compat.h"

namespace ORB_SLAM2 {

inline void FillTcim(const cv::Mat& Rcam12, const cv::Mat& tcam12, float Tcim[2][16]) {
    cv::Mat Tcam21 = cv::Mat::zeros(4, 4, CV_32F);
    cv::Mat Rcam21 = Rcam12.t();
    cv::Mat tcam21 = -Rcam21 * tcam12;
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) Tcam21.at<float>(r, c) = Rcam21.at<float>(r, c); Tcam21.at<float>(r, 3) = tcam21.at<float>(r); }
    Tcam21.at<float>(3, 3) = 1.0;
    cv::Mat Tcam11 = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { Tcim[0][4 * r + c] = Tcam11.at<float>(r, c); Tcim[1][4 * r + c] = Tcam21.at<float>(r, c); }
}

}  // namespace ORB_SLAM2

#endif
