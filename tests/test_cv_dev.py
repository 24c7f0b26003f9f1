"""csrc/cv_dev.h (the OpenCV operations as the kernels and the host routines of the library run them) against host/cv_compat.h (the
OpenCV stand-in the host classes and their drivers compute with): two restatements of the same OpenCV paths, written apart on purpose,
tied here directly and bit for bit -- until now only through the Python models.  One small program, plain g++ with the library's float
model (-ffp-contract=off), over seeded random floats and the special values (+-0, denormals, +-inf, NaN, +-1, the largest and the
smallest normal float), alpha in {1, -1, 1/3, an arbitrary double}, beta in {0, 1}:
    cv_gemm3 (both forms, row strides 1, 3 and 4)   gemm_small_elem, len 3
    cv_scale / cv_scale_t                            ew_scale / the evaluated `alpha * M.t()`
    cv_norm3 / cv_dot3                               cv::norm / Mat::dot
    x86_nan(float) / x86_nan(double)                 0xffc00000 / 0xfff8000000000000, every other value unchanged
The NaN among the inputs is 0xffc00000, the one x86 itself makes from inf - inf or 0 * inf: where two NaNs of different bits meet in one
addition, which of them comes out depends on the operand order the compiler picks for a commutative operation -- a property of neither
restatement -- and with this input every NaN inside a computation has the same bits, so that NaN results are compared bit for bit too."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi_orb_slam_amd", "csrc")
HOST = os.path.join(ROOT, "multi_orb_slam_amd", "host")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include "cv_dev.h"
#include "cv_compat.h"

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static uint64_t bits(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 32); }

static const float SPECIAL[] = {0.0f, -0.0f, from_bits(1u), from_bits(0x80000001u), from_bits(0x007fffffu), from_bits(0x80012345u),
                                std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                                from_bits(0xffc00000u), 1.0f, -1.0f, std::numeric_limits<float>::max(),
                                std::numeric_limits<float>::min()};
static const int NS = sizeof(SPECIAL) / sizeof(SPECIAL[0]);
// one in four a special value; otherwise a float of moderate exponent (products and sums stay finite, roundings differ)
static float draw() {
    const uint32_t r = rnd();
    if ((r & 3u) == 0) return SPECIAL[(r >> 2) % NS];
    const uint32_t sign = (r >> 2) & 1u, expo = 117u + ((r >> 3) % 21u), mant = rnd() & 0x7fffffu;
    return from_bits(sign << 31 | expo << 23 | mant);
}

static long g_checked = 0, g_bad = 0;
template <typename T> static void same(T got, T want, const char* what) {
    ++g_checked;
    if (bits(got) != bits(want)) { if (++g_bad <= 20) printf("MISMATCH %s: %a / %a\n", what, (double)got, (double)want); }
}

int main() {
    const double ALPHA[] = {1.0, -1.0, 1.0 / 3, 0.78539816339744828e-3};
    const double BETA[] = {0.0, 1.0};
    const int STRIDE[] = {1, 3, 4};
    for (int it = 0; it < 20000; ++it) {
        float A[12], b[3];
        for (float& x : A) x = draw();
        for (float& x : b) x = draw();
        const float c = draw();
        for (double alpha : ALPHA)
            for (double beta : BETA)
                for (int sa : STRIDE) {
                    const float want = cv::gemm_small_elem(A, (size_t)sa, b, 1, 3, alpha, c, beta);
                    same(cv_gemm3(A, sa, b, alpha, c, beta), want, "cv_gemm3 (row)");
                    same(cv_gemm3(A[0], A[sa], A[2 * sa], b[0], b[1], b[2], alpha, c, beta), want, "cv_gemm3 (scalars)");
                }
        cv::Mat ma(1, 3, CV_32F), mb(1, 3, CV_32F);
        for (int k = 0; k < 3; ++k) { ma.at<float>(0, k) = A[k]; mb.at<float>(0, k) = b[k]; }
        same(cv_norm3(A), cv::norm(ma), "cv_norm3");
        same(cv_dot3(A, b), ma.dot(mb), "cv_dot3");
        cv::Mat m3(3, 3, CV_32F);
        for (int k = 0; k < 9; ++k) m3.at<float>(k / 3, k % 3) = A[k];
        const double arbitrary = (double)draw() * 1.0000000000000002;
        const double alphas[] = {ALPHA[0], ALPHA[1], ALPHA[2], ALPHA[3], arbitrary};
        for (double alpha : alphas) {
            const cv::Mat s = cv::ew_scale(m3, alpha);
            const cv::Mat st = (alpha * m3.t()).eval();
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    same(cv_scale(A[3 * i + j], alpha), s.at<float>(i, j), "cv_scale");
                    same(cv_scale_t(A[3 * j + i], alpha), st.at<float>(i, j), "cv_scale_t");
                }
        }
    }
    // every special through the scaled-matrix forms with every weight
    for (float x : SPECIAL)
        for (double alpha : ALPHA) {
            cv::Mat m(1, 1, CV_32F);
            m.at<float>(0, 0) = x;
            same(cv_scale(x, alpha), cv::ew_scale(m, alpha).at<float>(0, 0), "cv_scale (special)");
            same(cv_scale_t(x, alpha), (alpha * m.t()).eval().at<float>(0, 0), "cv_scale_t (special)");
        }
    // x86_nan: every NaN becomes the one x86 makes from an invalid operation, everything else passes
    const uint32_t fnan[] = {0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xffffffffu, 0x7fc12345u};
    for (uint32_t u : fnan) same(x86_nan(from_bits(u)), from_bits(0xffc00000u), "x86_nan(float)");
    const uint64_t dnan[] = {0x7ff8000000000000ull, 0xfff8000000000000ull, 0x7ff0000000000001ull, 0xffffffffffffffffull};
    for (uint64_t u : dnan) {
        double d, want; const uint64_t w = 0xfff8000000000000ull;
        memcpy(&d, &u, 8); memcpy(&want, &w, 8);
        same(x86_nan(d), want, "x86_nan(double)");
    }
    for (float x : SPECIAL) if (x == x) { same(x86_nan(x), x, "x86_nan(float) passes"); same(x86_nan((double)x), (double)x, "x86_nan(double) passes"); }
    printf("checked %ld, mismatches %ld\n", g_checked, g_bad);
    return g_bad ? 1 : 0;
}
"""


def test_cv_dev_agrees_with_cv_compat_bit_for_bit(tmp_path):
    src = tmp_path / "cv_dev_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "cv_dev_check"
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", CSRC, "-I", HOST, "-o", str(exe), str(src)],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:])
    assert run.returncode == 0, run.stdout[-4000:]
    assert "mismatches 0" in run.stdout and "checked 0," not in run.stdout
