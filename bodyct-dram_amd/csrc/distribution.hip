// Lesion distribution report at inference (gfx950): per label of a label volume, the reduction of a depth map (the distance of
// every voxel from the lung surface, dram_edt) and of the voxel positions in one pass -- count, a fixed-point depth sum, the
// minimum and maximum depth as bit patterns, the sums of the voxel indices, a depth histogram in the row layout of
// dram_hist_summary and the counts per positional zone of a box.  Everything is integers: sums, minima and maxima by integer
// atomics and integer reductions, so no result depends on the order in which they land (the same bits every run).
//
// dram_label_depth is a streaming report of label_stream.h, which describes its two regimes; dram_label_depth_plan chooses
// between them from (label_kind, n, nbins, nzones) alone: the table of a call is n * (11 + nbins + 2 + nzones) 32-bit words.
// A group of 16 voxels may cross the end of a row and of a plane: the position of its first voxel is decoded by division and
// carried from voxel to voxel.  The zone of an index along an axis is the number of zone thresholds at or below it (at most 7,
// formed on the host from the box), which is the clamped quotient of the definition without a division.
#include "label_stream.h"

namespace dram {

constexpr int DEPTH_MAX_AXIS_ZONES = 8;
constexpr unsigned DEPTH_INF_BITS = 0x7f800000u;
constexpr int DEPTH_NO_THRESHOLD = INT32_MAX;  // no voxel index reaches it: D * H * W < 2^31

struct DepthArgs {
    const float* depth;
    const void* labels;
    const uint8_t* mask;
    unsigned long long *count, *qsum;
    unsigned *dmin, *dmax;
    unsigned long long *possum, *hist, *zones;
    int n, nbins, nzt;                        // nzt: entries of a zones row
    float bins_per_mm;
    int ny, nx;                               // zones along y and x (those along z only enter through tz)
    int tz[DEPTH_MAX_AXIS_ZONES - 1], ty[DEPTH_MAX_AXIS_ZONES - 1], tx[DEPTH_MAX_AXIS_ZONES - 1];
    unsigned H, W, HW;
    long long nvox, groups;                   // groups of 16 voxels taken with 16-byte loads; the rest goes voxel by voxel
};

__global__ __launch_bounds__(256) void depth_init_kernel(unsigned long long* __restrict__ count, unsigned long long* __restrict__ qsum,
                                                         unsigned* __restrict__ dmin, unsigned* __restrict__ dmax,
                                                         unsigned long long* __restrict__ possum, unsigned long long* __restrict__ hist,
                                                         unsigned long long* __restrict__ zones, int n, long long nhist, long long nzones) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { count[i] = 0; qsum[i] = 0; dmin[i] = DEPTH_INF_BITS; dmax[i] = 0; }
    if (i < 3LL * n) possum[i] = 0;
    if (hist && i < nhist) hist[i] = 0;
    if (zones && i < nzones) zones[i] = 0;
}

// the comparison comes before the conversion: +inf and everything at or above nbins / bins_per_mm go to the overflow entry
__device__ __forceinline__ int depth_bin(float d, float bins_per_mm, int nbins) {
    const float b = d * bins_per_mm;         // bins_per_mm is a power of two: exact
    return b >= (float)nbins ? nbins + 1 : 1 + (int)b;
}

// 2^21 * 2^10 = 2^31 at most: the product is exact and fits the unsigned conversion
__device__ __forceinline__ unsigned depth_q(float d) { return (unsigned)(fminf(d, 2097152.0f) * 1024.0f); }

__device__ __forceinline__ int depth_axis_zone(int i, const int (&t)[DEPTH_MAX_AXIS_ZONES - 1]) {
    int s = 0;
#pragma unroll
    for (int j = 0; j < DEPTH_MAX_AXIS_ZONES - 1; ++j) s += i >= t[j];
    return s;
}

// The position of a voxel and its zone, carried along the flat index.
template <bool ZONES>
struct DepthPos {
    unsigned z, y, x;
    int zz, zy, zx;
    __device__ __forceinline__ DepthPos(const DepthArgs& a, unsigned e) {
        z = e / a.HW;
        const unsigned r = e - z * a.HW;
        y = r / a.W;
        x = r - y * a.W;
        zz = zy = zx = 0;
        if (ZONES) {
            zz = depth_axis_zone((int)z, a.tz);
            zy = a.ny > 1 ? depth_axis_zone((int)y, a.ty) : 0;
            zx = a.nx > 1 ? depth_axis_zone((int)x, a.tx) : 0;
        }
    }
    __device__ __forceinline__ void step(const DepthArgs& a) {
        if (++x == a.W) {
            x = 0;
            if (++y == a.H) {
                y = 0;
                ++z;
                if (ZONES) zz = depth_axis_zone((int)z, a.tz);
            }
            if (ZONES) zy = a.ny > 1 ? depth_axis_zone((int)y, a.ty) : 0;
        }
        if (ZONES) zx = a.nx > 1 ? depth_axis_zone((int)x, a.tx) : 0;
    }
    __device__ __forceinline__ int zone(const DepthArgs& a) const { return (zz * a.ny + zy) * a.nx + zx; }
};

// Per label: count, minimum and maximum depth as bit patterns, the sums {fixed-point depth, z, y, x}, and two count tables, the
// depth histogram and the zones.
struct DepthPolicy {
    using Args = DepthArgs;
    using Value = unsigned;
    static constexpr int SUMS = 4, TABLES = 2;
    static constexpr unsigned MIN0 = DEPTH_INF_BITS, MAX0 = 0;
    __device__ __forceinline__ static int row(const DepthArgs& a, int t) { return t == 0 ? (a.hist ? a.nbins + 2 : 0) : (a.zones ? a.nzt : 0); }
    __device__ __forceinline__ static unsigned long long* table(const DepthArgs& a, int t) { return t == 0 ? a.hist : a.zones; }
    template <class Moments>
    __device__ __forceinline__ static void send(const DepthArgs& a, int label, const Moments& m) {
        const int k = label - 1;
        atomicAdd(&a.count[k], (unsigned long long)m.cnt);
        if (m.s[0]) atomicAdd(&a.qsum[k], m.s[0]);
        atomicMin(&a.dmin[k], m.mn);
        atomicMax(&a.dmax[k], m.mx);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (m.s[1 + c]) atomicAdd(&a.possum[3 * (size_t)k + c], m.s[1 + c]);
    }
};

template <class Acc, class LabelT, bool HIST, bool ZONES>
__global__ __launch_bounds__(1024) void label_depth_kernel(const DepthArgs a) {
    Acc acc(a);
    const auto add = [&](int l, float d, const DepthPos<ZONES>& p) {
        if (!(d >= 0.0f) || !acc.enter(l)) return;
        acc.m.see(__float_as_uint(d));
        acc.m.s[0] += depth_q(d);
        acc.m.s[1] += p.z; acc.m.s[2] += p.y; acc.m.s[3] += p.x;
        if (HIST) acc.count(0, (l - 1) * (a.nbins + 2) + depth_bin(d, a.bins_per_mm, a.nbins));
        if (ZONES) acc.count(1, (l - 1) * a.nzt + p.zone(a));
    };
    stream_labels<LabelT>(
        a.labels, a.mask, a.groups, a.nvox, acc,
        [&](long long g, const int (&l)[16]) {
            float d[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 v = reinterpret_cast<const float4*>(a.depth)[g * 4 + j];
                d[4 * j] = v.x; d[4 * j + 1] = v.y; d[4 * j + 2] = v.z; d[4 * j + 3] = v.w;
            }
            DepthPos<ZONES> p(a, (unsigned)(g * 16));
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                add(l[k], d[k], p);
                if (k < 15) p.step(a);
            }
        },
        [&](long long e, int l) { add(l, a.depth[e], DepthPos<ZONES>(a, (unsigned)e)); });
}

static inline bool depth_shape_ok(int label_kind, int n, int nbins, int nzones) {
    return label_kind_ok(label_kind, n) && hist_shape_ok(n, nbins) && nzones >= 0 &&
           nzones <= DEPTH_MAX_AXIS_ZONES * DEPTH_MAX_AXIS_ZONES * DEPTH_MAX_AXIS_ZONES && (int64_t)n * (nzones > 3 ? nzones : 3) < (1LL << 31);
}

static inline int64_t depth_table_words(int n, int nbins, int nzones) {
    return (int64_t)n * (label_moment_words<DepthPolicy>() + (nbins > 0 ? nbins + 2 : 0) + nzones);
}

static inline bool depth_bins_per_mm_ok(int b) { return b == 1 || b == 2 || b == 4 || b == 8 || b == 16; }

// The zone of index i along an axis with the box [a0, a1) and nz zones is ((clamp(i, a0, a1 - 1) - a0) * nz) / (a1 - a0), which
// is the number of j in 1 .. nz - 1 with clamp(i) - a0 >= ceil(j * (a1 - a0) / nz).  A threshold that the clamped index cannot
// reach (more zones than the box has voxels) is set out of reach, and the clamp is then no longer needed.
static inline void depth_thresholds(int a0, int a1, int nz, int (&t)[DEPTH_MAX_AXIS_ZONES - 1]) {
    const int64_t ext = (int64_t)a1 - a0;
    for (int j = 1; j < DEPTH_MAX_AXIS_ZONES; ++j) {
        const int64_t b = (int64_t)a0 + (j * ext + nz - 1) / nz;
        t[j - 1] = (j < nz && b <= (int64_t)a1 - 1) ? (int)b : DEPTH_NO_THRESHOLD;
    }
}

template <class Acc, class LabelT>
static int depth_launch(const DepthArgs& a, const StreamLaunch& g, hipStream_t st) {
    const char* who = "label_depth";
    if (a.hist) return a.zones ? launch_stream<label_depth_kernel<Acc, LabelT, true, true>>(a, g, st, who)
                               : launch_stream<label_depth_kernel<Acc, LabelT, true, false>>(a, g, st, who);
    return a.zones ? launch_stream<label_depth_kernel<Acc, LabelT, false, true>>(a, g, st, who)
                   : launch_stream<label_depth_kernel<Acc, LabelT, false, false>>(a, g, st, who);
}

template <class Acc>
static int depth_launch(const DepthArgs& a, int label_kind, const StreamLaunch& g, hipStream_t st) {
    return label_kind == 0 ? depth_launch<Acc, uint8_t>(a, g, st) : depth_launch<Acc, int32_t>(a, g, st);
}

}  // namespace dram

using namespace dram;

#define DEPTH_SHAPE_MSG "label_depth: label_kind 0 (uint8, n <= 255) or 1 (int32), n >= 1, nbins in 0..%d, nzones in 0..512, every table below 2^31 words"

extern "C" int dram_label_depth_plan(int label_kind, int n, int nbins, int nzones) {
    DRAM_REQUIRE(depth_shape_ok(label_kind, n, nbins, nzones), DEPTH_SHAPE_MSG, LABEL_MAX_BINS);
    return label_regime(depth_table_words(n, nbins, nzones));
}

extern "C" int dram_label_depth(const float* depth, const void* labels, int label_kind, const uint8_t* mask, int n, int64_t* count,
                                int64_t* qsum, uint32_t* dmin, uint32_t* dmax, int64_t* possum, int64_t* hist, int bins_per_mm, int nbins,
                                int64_t* zones, const int32_t* box, int nz, int ny, int nx, int D, int H, int W, void* stream) {
    DRAM_REQUIRE(depth && labels && count && qsum && dmin && dmax && possum, "label_depth: null pointer");
    DRAM_REQUIRE(D >= 1 && H >= 1 && W >= 1 && (int64_t)D * H * W < (1LL << 31), "label_depth: D, H, W >= 1 and D * H * W < 2^31");
    DRAM_REQUIRE(nz >= 1 && nz <= DEPTH_MAX_AXIS_ZONES && ny >= 1 && ny <= DEPTH_MAX_AXIS_ZONES && nx >= 1 && nx <= DEPTH_MAX_AXIS_ZONES,
                 "label_depth: nz, ny, nx must each be in 1..%d", DEPTH_MAX_AXIS_ZONES);
    const int nzt = nz * ny * nx;
    DRAM_REQUIRE((zones == nullptr) == (nzt == 1 && box == nullptr),
                 "label_depth: zones and its box go together (zones NULL iff nz * ny * nx == 1 and box NULL)");
    DRAM_REQUIRE(depth_shape_ok(label_kind, n, nbins, zones ? nzt : 0), DEPTH_SHAPE_MSG, LABEL_MAX_BINS);
    DRAM_REQUIRE((hist == nullptr) == (nbins == 0), "label_depth: hist and nbins go together (NULL iff 0)");
    DRAM_REQUIRE(nbins == 0 || depth_bins_per_mm_ok(bins_per_mm), "label_depth: bins_per_mm must be 1, 2, 4, 8 or 16");
    DRAM_REQUIRE(!box || (box[0] < box[1] && box[2] < box[3] && box[4] < box[5]), "label_depth: an empty box (a0 >= a1 on an axis)");
    DRAM_REQUIRE(((uintptr_t)depth & 3) == 0 && (label_kind == 0 || ((uintptr_t)labels & 3) == 0), "label_depth: misaligned depth or labels");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nvox = (int64_t)D * H * W;
    const int64_t nhist = hist ? (int64_t)n * (nbins + 2) : 0, nzones = zones ? (int64_t)n * nzt : 0;
    int64_t total = 3LL * n;
    total = nhist > total ? nhist : total;
    total = nzones > total ? nzones : total;
    hipLaunchKernelGGL(depth_init_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, (unsigned long long*)count,
                       (unsigned long long*)qsum, dmin, dmax, (unsigned long long*)possum, (unsigned long long*)hist,
                       (unsigned long long*)zones, n, (long long)nhist, (long long)nzones);
    const bool vec = aligned16(depth) && aligned16(labels) && (!mask || aligned16(mask));
    DepthArgs a{};
    a.depth = depth; a.labels = labels; a.mask = mask;
    a.count = (unsigned long long*)count; a.qsum = (unsigned long long*)qsum; a.dmin = dmin; a.dmax = dmax;
    a.possum = (unsigned long long*)possum; a.hist = (unsigned long long*)hist; a.zones = (unsigned long long*)zones;
    a.n = n; a.nbins = nbins; a.nzt = nzt; a.bins_per_mm = (float)(nbins > 0 ? bins_per_mm : 1); a.ny = ny; a.nx = nx;
    const int32_t whole[6] = {0, D, 0, H, 0, W};           // zones without a box: the zones of the whole volume
    const int32_t* b = box ? box : whole;
    depth_thresholds(b[0], b[1], nz, a.tz);
    depth_thresholds(b[2], b[3], ny, a.ty);
    depth_thresholds(b[4], b[5], nx, a.tx);
    a.H = (unsigned)H; a.W = (unsigned)W; a.HW = (unsigned)((int64_t)H * W);
    a.nvox = nvox; a.groups = vec ? nvox / 16 : 0;
    const int64_t words = depth_table_words(n, nbins, zones ? nzt : 0);
    const StreamLaunch g = stream_geometry(words, nvox, a.groups, 4096);
    const int rc = label_regime(words) == LABEL_LDS ? depth_launch<LdsLabelAcc<DepthPolicy>>(a, label_kind, g, st)
                                                    : depth_launch<WaveLabelAcc<DepthPolicy>>(a, label_kind, g, st);
    if (rc != DRAM_OK) return rc;
    return check_launch("label_depth");
}
