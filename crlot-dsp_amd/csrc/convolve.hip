// convolve.hip -- the frequency-domain delay line of partitioned FFT convolution
// (crlot_fdl_mac, crlot_convolve; the value contract is in include/crlot_dsp.h,
// "partitioned FFT convolution"): per bin, a complex FIR along the frame axis over
// the P partition spectra of the filter,
//   out[s][f][b] = sum over j = max(0, f-P+1) .. min(f, F_in-1), ascending, of
//                  H[(first_stream + s) mod n_filters][f-j][b] * X[s][j][b],
// four fmaf per term in the contract's order, one independent chain per output.
//
// K_fdl_mac  k_fdl_mac<R>: one wave owns 64 adjacent bins of one stream (phase_voc.hip's
//            organisation: a spectrum row is one coalesced 512-byte load) and one
//            chunk of output frames, which it walks in tiles of R frames.  A lane
//            keeps the tile's R complex accumulators and a window of R filter rows
//            in registers and walks the input frames f-P+1 .. f+R-1 once, in blocks
//            of R: each block loads R rows of X and R rows of H and feeds R x R
//            terms, so an interior block is 4 R^2 fmaf to 2 R loads (R = 8: 256 to
//            16).  The window slides by one filter row per input frame; unrolled by
//            R, the rotation is a renaming, no moves.  Every (input frame, output
//            frame) pair of a block is wave-uniform, so the blocks at a tile's ends,
//            where some pairs fall outside [0, P) or [0, F_in), skip them on scalar
//            branches and load nothing for them; rows are never padded with zeros
//            (a zero times a NaN of X would not be a zero).  H comes from L2 / L1:
//            at R = 8 that is one 8-byte load per 32 fmaf, and LDS would add a
//            stage and a barrier for nothing.  No scratch, no LDS.
//            R follows P: 1 and 2 for P = 1 and P <= 3 (one or two terms per
//            output: the memory-bound shapes run no tile machinery), 4 below
//            P = 12, 8 from there.  Chunks split a stream's output frames across
//            waves when streams x bin blocks alone would leave compute units idle; a
//            chunk re-reads the P - 1 input frames before it and recomputes nothing.
// Each output is its own chain in the order of the contract whatever R, the chunk
// and the block boundaries are, so the bits depend on none of them.
#include <algorithm>
#include <cstdint>

#include "launch_common.h"

namespace crlot {

namespace {

constexpr int kFW = 4;         // waves per workgroup
constexpr int kMinChunk = 32;  // the shortest chunk the policy makes (the knob may force shorter ones)

struct FdlKArgs {
    FdlArgs v;
    int64_t waves;
    int32_t nbw;  // column blocks per row, ceil(bins / 64)
    int32_t n_chunks, M;
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ void mac(float& re, float& im, float2 h, float2 x) {
    re = __builtin_fmaf(h.x, x.x, re);
    re = __builtin_fmaf(-h.y, x.y, re);
    im = __builtin_fmaf(h.x, x.y, im);
    im = __builtin_fmaf(h.y, x.x, im);
}

// Input frames j .. j+R-1 (j >= 0) against the tile's outputs ft .. ft+R-1, p0 = ft - j.
// On entry hw[k] = H[p0 + k] for k = 1 .. R-1 where that row exists; on exit the same
// for p0 - R.  Step u loads H[p0 - u] into the slot whose row left the window
// (slot 0 at u = 0) and pairs input frame j + u with output r through
// H[p0 - u + r], which is slot (r - u) mod R.  EDGE: some pairs or rows of the block
// do not exist; they are skipped and not loaded.
template <int R, bool EDGE>
__device__ __forceinline__ void block(const float2* __restrict__ X, int64_t ldx2, const float2* __restrict__ Hq,
                                      int64_t ldh2, int64_t j, int p0, int64_t F_in, int P, float (&re)[R],
                                      float (&im)[R], float2 (&hw)[R]) {
    float2 x[R], hn[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
        x[u] = float2{0.0f, 0.0f};
        hn[u] = float2{0.0f, 0.0f};
        const int p = p0 - u;  // the row entering the window; outputs pair with rows p .. p+R-1
        if (!EDGE || (j + u < F_in && p + R - 1 >= 0 && p <= P - 1)) x[u] = X[(j + u) * ldx2];
        if (!EDGE || (p >= 0 && p < P)) hn[u] = Hq[int64_t(p) * ldh2];
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
        hw[(R - u) % R] = hn[u];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int p = p0 - u + r;
            if (!EDGE || (j + u < F_in && p >= 0 && p < P)) mac(re[r], im[r], hw[(r - u + R) % R], x[u]);
        }
    }
}

template <int R>
__global__ __launch_bounds__(64 * kFW) void k_fdl_mac(const FdlKArgs a) {
    const FdlArgs& v = a.v;
    const int lane = threadIdx.x & 63;
    const int wave = uni(int(threadIdx.x >> 6));
    const int64_t gw = int64_t(blockIdx.x) * kFW + wave;
    if (gw >= a.waves) return;
    const int bw = int(gw % a.nbw);
    const int64_t sc = gw / a.nbw;
    const int c = int(sc % a.n_chunks);
    const int64_t s = sc / a.n_chunks;
    const int b = bw * 64 + lane;
    const bool live = b < v.bins;
    const int bl = live ? b : v.bins - 1;
    const int P = v.P;
    const int64_t F_in = v.F_in;
    const float2* X = reinterpret_cast<const float2*>(v.in + s * v.ld_in) + bl;
    const int64_t ldx2 = v.ldf_in / 2;
    const int64_t ldh2 = v.ldh2;
    const int64_t q = (s + v.first_stream) % v.n_filters;
    const float2* Hq = reinterpret_cast<const float2*>(v.h) + q * P * ldh2 + bl;
    float2* O = reinterpret_cast<float2*>(v.out + s * v.ld_out) + bl;
    const int64_t ldo2 = v.ldf_out / 2;
    const int64_t f0 = int64_t(c) * a.M;
    const int64_t f1 = f0 + a.M < v.F_out ? f0 + a.M : v.F_out;

    for (int64_t ft = f0; ft < f1; ft += R) {
        float re[R], im[R];
        float2 hw[R];
#pragma unroll
        for (int r = 0; r < R; ++r) re[r] = im[r] = 0.0f;
        // input frames [js, je]: those any output of the tile pairs with
        const int64_t js = ft - P + 1 > 0 ? ft - P + 1 : 0;
        const int64_t je = ft + R - 1 < F_in - 1 ? ft + R - 1 : F_in - 1;
        int p0 = int(ft - js);  // <= P - 1
#pragma unroll
        for (int k = 1; k < R; ++k) {
            hw[k] = float2{0.0f, 0.0f};
            if (p0 + k < P) hw[k] = Hq[int64_t(p0 + k) * ldh2];
        }
        hw[0] = float2{0.0f, 0.0f};
        for (int64_t j = js; j <= je; j += R, p0 -= R) {
            if (j + R - 1 < F_in && p0 - (R - 1) >= 0 && p0 + R - 1 <= P - 1)
                block<R, false>(X, ldx2, Hq, ldh2, j, p0, F_in, P, re, im, hw);
            else
                block<R, true>(X, ldx2, Hq, ldh2, j, p0, F_in, P, re, im, hw);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (live && ft + r < f1) O[(ft + r) * ldo2] = float2{re[r] + 0.0f, im[r] + 0.0f};
    }
}

template <int R>
int64_t resident_waves() {
    static const int per_cu = [] {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(k_fdl_mac<R>), 64 * kFW,
                                                         0) != hipSuccess ||
            nb <= 0)
            nb = 1;
        return nb * kFW;
    }();
    return int64_t(per_cu) * device_cus();
}

// About two resident rounds of waves, chunks of at least kMinChunk output frames and
// whole tiles; the knob forces min(chunks, F_out) chunks of any length.
template <int R>
hipError_t launch(FdlKArgs& a, int chunks, crlot_convolver_launch* rec, hipStream_t stream) {
    const FdlArgs& v = a.v;
    const int64_t units = int64_t(v.n_streams) * a.nbw;
    int64_t n, m;
    if (chunks > 0) {
        n = std::min<int64_t>(chunks, v.F_out);
        m = (v.F_out + n - 1) / n;
    } else {
        n = (2 * resident_waves<R>() + units - 1) / units;
        n = std::max<int64_t>(1, std::min<int64_t>(n, v.F_out / kMinChunk));
        m = ((v.F_out + n - 1) / n + R - 1) / R * R;
    }
    a.M = int32_t(m);
    a.n_chunks = int32_t((v.F_out + m - 1) / m);
    a.waves = units * a.n_chunks;
    const int64_t grid = (a.waves + kFW - 1) / kFW;
    if (grid > INT32_MAX) return hipErrorInvalidValue;
    if (rec) {
        *rec = crlot_convolver_launch{};
        rec->kernel = CRLOT_K_FDL_MAC;
        rec->threads = 64 * kFW;
        rec->grid = grid;
        rec->n_chunks = a.n_chunks;
        rec->chunk = a.M;
        rec->tile = R;
    }
    return fk::launch_kernel_plain(k_fdl_mac<R>, CRLOT_K_FDL_MAC, dim3(unsigned(grid)), dim3(64 * kFW), 0, stream, a);
}

}  // namespace

hipError_t launch_fdl_mac(const FdlArgs& v, int chunks, crlot_convolver_launch* rec, hipStream_t stream) {
    if (v.n_streams <= 0 || v.F_out <= 0 || v.F_in < 0 || v.F_in > INT32_MAX || v.F_out > INT32_MAX || v.bins <= 0 ||
        v.P <= 0 || v.n_filters <= 0 || v.ldh2 < v.bins || !v.in || !v.out || !v.h || (v.ldf_in & 1) ||
        (v.ld_in & 1) || (v.ldf_out & 1) || (v.ld_out & 1) || v.ldf_in < 2 * int64_t(v.bins) ||
        v.ldf_out < 2 * int64_t(v.bins) || chunks < 0)
        return hipErrorInvalidValue;
    FdlKArgs a{};
    a.v = v;
    a.nbw = (v.bins + 63) / 64;
    if (v.P == 1) return launch<1>(a, chunks, rec, stream);
    if (v.P <= 3) return launch<2>(a, chunks, rec, stream);
    if (v.P < 12) return launch<4>(a, chunks, rec, stream);
    return launch<8>(a, chunks, rec, stream);
}

}  // namespace crlot
