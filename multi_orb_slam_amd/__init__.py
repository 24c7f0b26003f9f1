"""multi_orb_slam_amd -- MI355X-native ORB front end (ORBextractor + ORBmatcher hot path of Multi_ORB_SLAM).

The product is the C-ABI shared library `lib/libmorb.so` (hand-written HIP kernels for gfx950, declared in
include/orbx.h, orbm.h, orbf.h and orbv.h) plus the C++ host classes in `host/` that keep the reference's
ORB_SLAM2::ORBextractor / ORBmatcher signatures.  This Python package is a thin ctypes mirror of that ABI used by
the tests, the benchmark and the multi-GPU driver; it contains no compute and no CPU fallback.
"""
from ._lib import lib, build, LIB_PATH, OrbError, KP_DTYPE, QUERY_DTYPE, POINT_DTYPE, TRACK_DTYPE, REFRESH_DTYPE  # noqa: F401
from .extractor import Extractor, ExtractorParams, tables  # noqa: F401
from .matcher import Matcher, FrameData, LocalPoints, View, descriptor_distance, three_maxima  # noqa: F401
from .matcher import frustum_host, level_thresholds, RefreshBatch, refresh_points_host  # noqa: F401
from .matcher import ResidentMap, local_map_vote_host, local_map_points_host  # noqa: F401
from ._lib import OBS_DTYPE, MAX_POINTS, MAP_MAX_KEYFRAMES, MAP_MAX_FEATURES, MAP_MAX_LOCAL, POINT_BAD  # noqa: F401
from .matcher import local_map_covisibility_host, local_map_culling_host  # noqa: F401
from ._lib import COVIS_DTYPE, FEATURE_LEVEL_MASK, FEATURE_FAR  # noqa: F401
from .matcher import local_map_correct_sim3_host, local_map_correct_rigid_host  # noqa: F401
from ._lib import CORRECT_DTYPE  # noqa: F401
from .matcher import PoseProblem, pose_optimize_host, pose_sincos  # noqa: F401
from ._lib import POSE_PROBLEM_DTYPE, POSE_RESULT_DTYPE, POSE_CAM0, POSE_ALL_CAMS, POSE_ORDER_INDEX, POSE_ORDER_DEVICE, POSE_CAP  # noqa: F401
from .matcher import Sim3Problem, sim3_ransac_host, sim3_walk, sim3_iterations, sim3_atan2  # noqa: F401
from ._lib import SIM3_PROBLEM_DTYPE, SIM3_HYP_DTYPE, SIM3_MATH_LIBM, SIM3_MATH_DEVICE, SIM3_CAP, SIM3_MAX_ITS, SIM3_MAX_BATCH  # noqa: F401
from .matcher import Sim3OptProblem, sim3_optimize_host, sim3opt_exp, sim3opt_expmap, sim3opt_ldlt7  # noqa: F401
from .matcher import LocalBAProblem, LocalBAResult, local_ba_host, lba_edge_eval, lba_controller_trace, lba_ldlt  # noqa: F401
from ._lib import LBA_MAX_FREE, LBA_MAX_POSES, LBA_MAX_POINTS, LBA_MAX_EDGES, LBA_ENDED_COMPLETE, LBA_ENDED_STOPPED_AT_START  # noqa: F401
from ._lib import LBA_ENDED_NO_SECOND, LBA_FLAG_LEVEL1, LBA_FLAG_ERASE  # noqa: F401
from .matcher import GlobalBAResult, bundle_adjust_host, ba_ldlt  # noqa: F401
from ._lib import BA_MAX_FREE, BA_MAX_POSES, BA_MAX_POINTS, BA_MAX_EDGES, BA_PANEL  # noqa: F401
from .matcher import EssentialGraphProblem, EssentialGraphResult, essential_graph_host, eg_edge_eval, sim3_log_eval  # noqa: F401
from .matcher import pose_acos, pose_log  # noqa: F401
from ._lib import EG_MAX_FREE, EG_MAX_VERTICES, EG_MAX_EDGES, EG_MAX_POINTS  # noqa: F401
from ._lib import SIM3OPT_PROBLEM_DTYPE, SIM3OPT_RESULT_DTYPE, SIM3OPT_CAP, SIM3OPT_MAX_BATCH  # noqa: F401
from .matcher import PnPProblem, pnp_ransac_host, pnp_walk, pnp_walk_state, pnp_parameters, pnp_svd, pnp_qr_solve, pnp_compute_pose  # noqa: F401
from ._lib import PNP_PROBLEM_DTYPE, PNP_HYP_DTYPE, PNP_REFINED_DTYPE, PNP_WALK_DTYPE, PNP_CAP, PNP_MAX_ITS, PNP_MAX_BATCH, PNP_MAX_RECORDS  # noqa: F401
from ._lib import PNP_FLAG_SINGULAR_QR, PNP_FLAG_RANDOM_SVD, PNP_WALK_NOTHING, PNP_WALK_REFINED, PNP_WALK_BEST  # noqa: F401
from .vocabulary import Vocabulary, BowSearch, Side as BowSide, FeatureVector, score_l1, KeyFrameDatabase  # noqa: F401
from .vocabulary import TriKeyframe, TRI_OUT_DTYPE, cos_stereo, triangulate_pairs_host, NewPointsRound  # noqa: F401
