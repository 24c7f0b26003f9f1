// EssentialGraph.cc -- Optimizer::OptimizeEssentialGraph (host/Optimizer.h; reference src/Optimizer.cc:1373-1677) over
// orbm_essential_graph (include/orbm.h).  Steps 2-4 (the vertices, the loop edges, the spanning-tree / loop / covisibility edges with
// their measurements Sjw * Swi in double) and steps 6-7 (SetPose under mMutexMapUpdate, SetWorldPos, UpdateNormalAndDepth) are the
// reference's statement by statement; the g2o graph, its optimisation and the arithmetic of steps 6 and 7 are the arrays of one call.
// What differs from the reference is the call's (include/orbm.h: the dense solver) and two places where the reference dereferences
// a NULL vertex: an edge with an end that has no vertex (a bad keyframe) is not added -- nor entered into sInsertedEdges -- and a bad
// keyframe of vpKFs gets no SetPose; vCorrectedSwc of such a keyframe stays default-constructed, like its vScw.
#ifdef MORB_USE_REFERENCE_TYPES
#include "LoopClosing.h"
#endif
#include "Optimizer.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <vector>
#include "../../include/orbm.h"
#include "g2o_compat.h"
#include "slam_types.h"
#ifdef MORB_USE_REFERENCE_TYPES
#include "Map.h"
#endif
#include "MapPointRefresh.h"

namespace ORB_SLAM2 {

// tools/essential_graph_bench.py on an MI355X (profiles/r22/essential_graph_bench.json): at 120 edges (30 free keyframes) the host
// routine takes 4.9 ms against the device call's 8.0 ms, at 161 edges (40) 11.8 against 11.0 ms, at 202 (50) 23.3 against 14.4 ms.  The
// two cross just below the 161-edge world.
const int EG_HOST_BELOW = 160;

namespace {
// Converter::toMatrix3d / toVector3d of the float matrices, g2o::Sim3(Rcw, tcw, 1.0)
g2o::Sim3 sim3_of_pose(KeyFrame* pKF) {
    const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation();
    g2o::Matrix3d Rcw;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rcw(r, c) = (double)R.at<float>(r, c);
    const g2o::Vector3d tcw((double)t.at<float>(0), (double)t.at<float>(1), (double)t.at<float>(2));
    return g2o::Sim3(Rcw, tcw, 1.0);
}
void push8(std::vector<double>& v, const g2o::Sim3& S) {
    const g2o::Quaterniond& q = S.rotation();
    v.push_back(q.x()); v.push_back(q.y()); v.push_back(q.z()); v.push_back(q.w());
    for (int k = 0; k < 3; ++k) v.push_back(S.translation()[k]);
    v.push_back(S.scale());
}
}  // namespace

void Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                                       const std::map<KeyFrame*, std::set<KeyFrame*> >& LoopConnections, const bool& bFixScale) {
    const std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
    const std::vector<MapPoint*> vpMPs = pMap->GetAllMapPoints();
    const unsigned int nMaxKFid = pMap->GetMaxKFid();
    std::vector<g2o::Sim3> vScw(nMaxKFid + 1);
    std::vector<int> vertex_of(nMaxKFid + 1, -1);          // optimizer.vertex(id): the index in the call's arrays, -1: NULL
    const int minFeat = 100;

    // Set KeyFrame vertices (:1414-1452).  The call wants the free ones first in ascending mnId, then the fixed one.
    std::vector<KeyFrame*> vpVertexKFs;
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrame* pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const int nIDi = pKF->mnId;
        LoopClosing::KeyFrameAndPose::const_iterator it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) vScw[nIDi] = it->second;
        else vScw[nIDi] = sim3_of_pose(pKF);
        if (pKF != pLoopKF) vpVertexKFs.push_back(pKF);
    }
    std::sort(vpVertexKFs.begin(), vpVertexKFs.end(), [](KeyFrame* a, KeyFrame* b) { return a->mnId < b->mnId; });
    const int n_free = (int)vpVertexKFs.size();
    for (size_t i = 0; i < vpKFs.size(); i++) if (!vpKFs[i]->isBad() && vpKFs[i] == pLoopKF) vpVertexKFs.push_back(vpKFs[i]);
    std::vector<double> vertex;
    for (size_t v = 0; v < vpVertexKFs.size(); ++v) { vertex_of[vpVertexKFs[v]->mnId] = (int)v; push8(vertex, vScw[vpVertexKFs[v]->mnId]); }

    std::vector<double> measurement;
    std::vector<int32_t> edge_v0, edge_v1;
    // addEdge with setVertex(0, vertex(nIDi)), setVertex(1, vertex(nIDj)); false: an end has no vertex, nothing is added
    auto add_edge = [&](long unsigned int nIDi, long unsigned int nIDj, const g2o::Sim3& Sji) -> bool {
        if (vertex_of[nIDi] < 0 || vertex_of[nIDj] < 0) return false;
        edge_v0.push_back(vertex_of[nIDi]); edge_v1.push_back(vertex_of[nIDj]);
        push8(measurement, Sji);
        return true;
    };
    std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;

    // Set Loop edges (:1461-1492)
    for (std::map<KeyFrame*, std::set<KeyFrame*> >::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
        KeyFrame* pKF = mit->first;
        const long unsigned int nIDi = pKF->mnId;
        const std::set<KeyFrame*>& spConnections = mit->second;
        const g2o::Sim3 Siw = vScw[nIDi];
        const g2o::Sim3 Swi = Siw.inverse();
        for (std::set<KeyFrame*>::const_iterator sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
            const long unsigned int nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight_cam1(*sit) < minFeat) continue;
            const g2o::Sim3 Sjw = vScw[nIDj];
            const g2o::Sim3 Sji = Sjw * Swi;
            if (!add_edge(nIDi, nIDj, Sji)) continue;
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }

    // Set normal edges (:1496-1613)
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrame* pKF = vpKFs[i];
        const int nIDi = pKF->mnId;
        g2o::Sim3 Swi;
        LoopClosing::KeyFrameAndPose::const_iterator iti = NonCorrectedSim3.find(pKF);
        if (iti != NonCorrectedSim3.end()) Swi = (iti->second).inverse();
        else Swi = vScw[nIDi].inverse();
        KeyFrame* pParentKF = pKF->GetParent();

        // Spanning tree edge
        if (pParentKF) {
            int nIDj = pParentKF->mnId;
            g2o::Sim3 Sjw;
            LoopClosing::KeyFrameAndPose::const_iterator itj = NonCorrectedSim3.find(pParentKF);
            if (itj != NonCorrectedSim3.end()) Sjw = itj->second;
            else Sjw = vScw[nIDj];
            g2o::Sim3 Sji = Sjw * Swi;
            add_edge(nIDi, nIDj, Sji);
        }

        // Loop edges
        const std::set<KeyFrame*> sLoopEdges = pKF->GetLoopEdges();
        for (std::set<KeyFrame*>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
            KeyFrame* pLKF = *sit;
            if (pLKF->mnId < pKF->mnId) {
                g2o::Sim3 Slw;
                LoopClosing::KeyFrameAndPose::const_iterator itl = NonCorrectedSim3.find(pLKF);
                if (itl != NonCorrectedSim3.end()) Slw = itl->second;
                else Slw = vScw[pLKF->mnId];
                g2o::Sim3 Sli = Slw * Swi;
                add_edge(nIDi, pLKF->mnId, Sli);
            }
        }

        // Covisibility graph edges
        const std::vector<KeyFrame*> vpConnectedKFs = pKF->GetCovisiblesByWeight_cam1(minFeat);
        for (std::vector<KeyFrame*>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
            KeyFrame* pKFn = *vit;
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    g2o::Sim3 Snw;
                    LoopClosing::KeyFrameAndPose::const_iterator itn = NonCorrectedSim3.find(pKFn);
                    if (itn != NonCorrectedSim3.end()) Snw = itn->second;
                    else Snw = vScw[pKFn->mnId];
                    g2o::Sim3 Sni = Snw * Swi;
                    add_edge(nIDi, pKFn->mnId, Sni);
                }
            }
        }
    }

    // the points of step 7 (:1646-1666): nIDr and GetWorldPos() are read before the call, nothing between here and there writes them
    std::vector<float> points;
    std::vector<int32_t> point_ref;
    std::vector<int> row_of(vpMPs.size(), -1);
    for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
        MapPoint* pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        int nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId) {
            nIDr = pMP->mnCorrectedReference;
        } else {
            KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
            nIDr = pRefKF->mnId;
        }
        row_of[i] = (int)point_ref.size();
        point_ref.push_back(nIDr >= 0 && (unsigned int)nIDr <= nMaxKFid ? vertex_of[nIDr] : -1);
        const cv::Mat P3Dw = pMP->GetWorldPos();
        for (int k = 0; k < 3; ++k) points.push_back(P3Dw.at<float>(k));
    }

    orbm_eg_problem P;
    std::memset(&P, 0, sizeof(P));
    P.n_free = n_free; P.n_vertices = (int32_t)vpVertexKFs.size(); P.n_edges = (int32_t)edge_v0.size(); P.n_points = (int32_t)point_ref.size();
    P.fix_scale = bFixScale ? 1 : 0;
    P.vertex = vertex.data(); P.measurement = measurement.data(); P.edge_v0 = edge_v0.data(); P.edge_v1 = edge_v1.data();
    P.points = points.data(); P.point_ref = point_ref.data();
    std::vector<double> estimate(8 * std::max<size_t>(vpVertexKFs.size(), 1));
    std::vector<float> Tiw(16 * std::max<size_t>(vpVertexKFs.size(), 1)), point_f(3 * std::max<size_t>(point_ref.size(), 1));
    orbm_eg_result R;
    std::memset(&R, 0, sizeof(R));
    R.estimate = estimate.data(); R.Tiw = Tiw.data(); R.point_f = point_f.data();

    // Optimize! (:1617-1618)
    ORBmatcher matcher(0.6f, false);                       // (the handle underneath is the calling thread's)
    int rc;
    if (P.n_edges < EG_HOST_BELOW || n_free == 0) {
        rc = orbm_essential_graph_host(&P, 20, ORBM_POSE_ORDER_DEVICE, &R);
    } else {
        orbm_matcher* h = matcher.GetDeviceHandle();
        if (!h) return;                                    // (reported by the matcher)
        rc = orbm_essential_graph(h, &P, 20, &R);
    }
    if (rc != ORB_OK) { std::fprintf(stderr, "OptimizeEssentialGraph: %s -- nothing optimised\n", orb_last_error()); return; }

    std::unique_lock<decltype(pMap->mMutexMapUpdate)> lock(pMap->mMutexMapUpdate);

    // SE3 Pose Recovering (:1624-1642)
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame* pKFi = vpKFs[i];
        const int nIDi = pKFi->mnId;
        if (vertex_of[nIDi] < 0) continue;                 // (a bad keyframe: the reference dereferences NULL here)
        const float* T = Tiw.data() + 16 * (size_t)vertex_of[nIDi];
        cv::Mat M(4, 4, CV_32F);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) M.at<float>(r, c) = T[4 * r + c];
        pKFi->SetPose(M);
    }

    // Correct points (:1646-1676): SetWorldPos in vpMPs' order; UpdateNormalAndDepth of all of them in one batched call
    std::vector<MapPoint*> vpRefresh;
    for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
        MapPoint* pMP = vpMPs[i];
        if (row_of[i] < 0) continue;
        const float* X = point_f.data() + 3 * (size_t)row_of[i];
        cv::Mat Pos(3, 1, CV_32F);
        for (int k = 0; k < 3; ++k) Pos.at<float>(k) = X[k];
        pMP->SetWorldPos(Pos);
        vpRefresh.push_back(pMP);
    }
    if (!vpRefresh.empty()) RefreshMapPoints(matcher, vpRefresh, REFRESH_NORMAL_DEPTH);
}

}  // namespace ORB_SLAM2
