// Device chunk loader (gfx950): the host side of a training step's first stage, batched and without host round trips.
//
// The reference prepares every chunk on the host in two places:
//   RadboudCOVIDLobeVesselChunk.get_data (dram/dataset.py:450-486): the pseudo-lesion label of the weak supervision,
//       w_scan = windowing(scan, to_span=(0, 1)); _, th = binary_cam(w_scan[lobe > 0], 0.75);
//       lesion_candidate = (w_scan > th) & (lobe > 0); vessel = (vessel > 0) & (lobe > 0)
//   LesionSegChunkTrain.preprocessing (dram/job_runner.py:586-597): Windowing(min, max) of "#image" as float32
//       (data_transforms.py:37-54), then Resample (data_transforms.py:65-211): linear for the image, nearest neighbour for every
//       "...reference" key, through sitk.ResampleImageFilter (utils.py:299-381; its grid: volume_math.h).
// Here the N chunks of a batch lie back to back in one buffer per kind (int16 scans, uint8 lobes, uint8 vessels), every chunk
// with its own size, described by a device table of ChunkRec; three entry points, none of which synchronises, allocates or
// reads per-sample data from the host:
//   chunk_hist256   per-sample 256-bin histogram of binary_cam's 8-bit view of the windowed scan inside the lobe (one launch)
//   otsu256         binary_cam's threshold from those histograms, on the device (one block per sample)
//   chunk_prepare   windowed + linearly resampled image, nearest-neighbour lobe / pseudo-lesion / vessel masks at the common
//                   output size, one launch, the pseudo-lesion mask never written at source resolution
#include "volume_math.h"

namespace dram {

struct ChunkRec {            // 48 bytes, mirrored by dram_amd/preprocess.py:TABLE_DTYPE
    long long off;           // first element of the chunk in the packed buffers
    int Di, Hi, Wi, pad;
    double sz, sy, sx;       // output-to-input index step per axis (required_spacing / spacing)
};
static_assert(sizeof(ChunkRec) == 48, "ChunkRec is part of the ABI");

// hist[n][b] = #{v in chunk n : lobe[v] > 0, scan_bin(windowed_scan(scan[v])) == b} (volume_math.h), as scan_hist_kernel (infer.hip).
// grid (blocks per sample, N).  The packed buffers are walked in groups of 8 elements aligned in BUFFER coordinates (the bases
// are 16-byte aligned, a chunk's offset is not): a group inside the chunk is one 16-byte scan load and one 8-byte lobe load, the
// two ragged groups at the chunk's ends go element by element.  One LDS histogram per wave (the lobe's values crowd a few
// bins), then one 64-bit integer atomic per occupied bin and block: integer sums, so the result does not depend on the order.
__global__ __launch_bounds__(256) void chunk_hist_kernel(const int16_t* __restrict__ scans, const uint8_t* __restrict__ lobes,
                                                         const ChunkRec* __restrict__ table,
                                                         unsigned long long* __restrict__ hist, int wmin, int wmax) {
    __shared__ unsigned lh[4][256];
    const int n = blockIdx.y;
    const ChunkRec r = table[n];
    if (r.Di <= 0 || r.Hi <= 0 || r.Wi <= 0) return;
    const long long lo = r.off, hi = r.off + (long long)r.Di * r.Hi * r.Wi;
    const long long g_lo = lo >> 3, g_hi = (hi + 7) >> 3;                       // groups [g_lo, g_hi)
    if (g_lo + (long long)blockIdx.x * 256 >= g_hi) return;                     // nothing for this block (uniform)
    for (int k = 0; k < 4; ++k) lh[k][threadIdx.x] = 0;
    __syncthreads();
    unsigned* mine = lh[threadIdx.x >> 6];
    const long long stride = (long long)gridDim.x * 256;
    for (long long g = g_lo + (long long)blockIdx.x * 256 + threadIdx.x; g < g_hi; g += stride) {
        const long long e0 = g << 3;
        if (e0 >= lo && e0 + 8 <= hi) {
            const uint2 lb = *reinterpret_cast<const uint2*>(lobes + e0);
            if ((lb.x | lb.y) == 0) continue;                                   // outside the lobe: the scan is not needed
            const uint4 sv = *reinterpret_cast<const uint4*>(scans + e0);
            const unsigned sw[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned l = ((k < 4 ? lb.x : lb.y) >> (8 * (k & 3))) & 0xffu;
                if (l) atomicAdd(&mine[scan_bin(windowed_scan((int)(int16_t)((sw[k >> 1] >> (16 * (k & 1))) & 0xffffu), wmin, wmax))], 1u);
            }
        } else {
            const long long a = e0 > lo ? e0 : lo, b = e0 + 8 < hi ? e0 + 8 : hi;
            for (long long e = a; e < b; ++e)
                if (lobes[e] > 0) atomicAdd(&mine[scan_bin(windowed_scan((int)scans[e], wmin, wmax))], 1u);
        }
    }
    __syncthreads();
    const unsigned long long c = (unsigned long long)lh[0][threadIdx.x] + lh[1][threadIdx.x] + lh[2][threadIdx.x] + lh[3][threadIdx.x];
    if (c) atomicAdd(&hist[(size_t)n * 256 + threadIdx.x], c);
}

// binary_cam's threshold (dram/utils.py:226-242) from the 8-bit histogram, exactly as inference.binary_cam_threshold /
// otsu_threshold_from_hist evaluate it in numpy: bins over the occupied range lo..hi; w1 / sum(h * centre) as fp64 running sums
// in ascending bin order, w2 / its weighted sum in descending order (np.cumsum is sequential); m = weighted sum / weight;
// var12[i] = w1[i] * w2[i+1] * (m1[i] - m2[i+1])^2 evaluated left to right, no fused multiply-add anywhere; the first maximum
// wins (np.argmax); th = min(t * scaler, 255) / 255.  Fewer than two occupied bins: th = bin / 255.  An empty histogram (an
// empty lobe) makes the reference raise IndexError; the device cannot raise without a synchronisation: th = +inf, which no
// voxel exceeds (documented deviation).  One block per sample; the two scans are 256 dependent fp64 adds each, done by one
// lane per direction.
__global__ __launch_bounds__(256) void otsu256_kernel(const unsigned long long* __restrict__ hist, double scaler,
                                                      double* __restrict__ th) {
#pragma clang fp contract(off)
    __shared__ double h[256], w1[256], s1[256], w2[256], s2[256];
    __shared__ int lo_s, hi_s, cnt_s;
    const int n = blockIdx.x, t = threadIdx.x;
    const unsigned long long c = hist[(size_t)n * 256 + t];
    h[t] = (double)c;
    if (t == 0) { lo_s = 256; hi_s = -1; cnt_s = 0; }
    __syncthreads();
    if (c) { atomicMin(&lo_s, t); atomicMax(&hi_s, t); atomicAdd(&cnt_s, 1); }
    __syncthreads();
    const int lo = lo_s, hi = hi_s;
    if (cnt_s < 2) {
        if (t == 0) th[n] = cnt_s == 0 ? __longlong_as_double(0x7ff0000000000000LL) : (double)lo / 255.0;
        return;
    }
    if (t == 0) {
        double w = 0.0, s = 0.0;
        for (int b = lo; b <= hi; ++b) {
            const double p = h[b] * (double)b;
            w = w + h[b]; s = s + p;
            w1[b] = w; s1[b] = s;
        }
    } else if (t == 64) {
        double w = 0.0, s = 0.0;
        for (int b = hi; b >= lo; --b) {
            const double p = h[b] * (double)b;
            w = w + h[b]; s = s + p;
            w2[b] = w; s2[b] = s;
        }
    }
    __syncthreads();
    if (t == 0) {
        int best = lo;
        double vbest = 0.0;
        for (int b = lo; b < hi; ++b) {
            const double m1 = s1[b] / w1[b], m2 = s2[b + 1] / w2[b + 1];
            const double d = m1 - m2;
            const double ww = w1[b] * w2[b + 1];
            const double dd = d * d;
            const double v = ww * dd;
            if (b == lo || v > vbest) { vbest = v; best = b; }
        }
        const double ts = (double)best * scaler;
        th[n] = (ts < 255.0 ? ts : 255.0) / 255.0;
    }
}

// ---- chunk_prepare
constexpr int PREP_MAX_ROWS = 64;      // output rows (z, y) per block
constexpr int PREP_MAX_WO = 2048;      // x table: 16 bytes per output column in dynamic LDS
struct PrepX {                          // per output column
    int x0, xn;                         // base voxel of the linear pair (upper = min(x0 + 1, Wi - 1)); nearest voxel, -1 = outside
    double tx;
};
struct PrepRow {                        // per output row of the block
    int z0, z1, zn, y0, y1, yn;         // zn / yn: nearest voxel, -1 = outside the buffer
    double tz, ty;
};
struct PrepArgs {
    const int16_t* scans;
    const uint8_t* lobes;
    const uint8_t* vessels;             // may be null
    const ChunkRec* table;
    const double* th;                   // may be null (no lesion output)
    float* image;
    float* lobe_out;
    float* lesion_out;                  // may be null
    float* vessel_out;                  // may be null
    int Do, Ho, Wo, rows;               // rows: output rows per block
    float wmin, wmax;
    int pwmin, pwmax;
};

// Windowing(min, max) of the scan cast to float32 (data_transforms.py:46-54 -> utils.windowing on a float32 array): clip,
// subtract, divide by float(max - min), * (1 - 0) + 0, every step rounded to fp32 (the last two change nothing: x * 1 = x and
// the quotient is never -0).  `/` is IEEE-rounded: the library is built without -ffast-math and hipcc's default for HIP is the
// correctly rounded fp32 division (v_div_scale / v_div_fmas / v_div_fixup in the ISA, not v_rcp alone).
__device__ __forceinline__ float window_f32(int16_t s, float wmin, float wmax, float range) {
#pragma clang fp contract(off)
    float v = (float)s;
    v = v < wmin ? wmin : (v > wmax ? wmax : v);
    return (v - wmin) / range;
}

// grid (row tiles, N), 256 threads.  A block owns `rows` consecutive output rows (z, y) of one sample: a contiguous span of every
// output.  It first fills the sample's x table (index pair, weight, nearest voxel per output column), the z / y entries of its
// rows (itk_axis, volume_math.h) and the pseudo-lesion cut into LDS -- per block, not per voxel --, then walks its span in quads aligned in OUTPUT
// coordinates: a quad inside the span is one 16-byte store per output, the ragged ends go element by element, so any Wo works.
// Per output voxel: the 8 scan neighbours of the linear cell (the nearest voxel is one of them), 1 lobe and 1 vessel value.
// Pseudo-lesion: (w_scan > th) with w_scan = windowed_scan(s, pwmin, pwmax) (volume_math.h).  That predicate is monotone in the clipped integer k = clip(s) - pwmin (a correctly rounded division by a
// positive constant is non-decreasing), so the block finds the smallest k whose quotient exceeds th by bisection with that very
// expression, and a voxel is a candidate iff its k reaches it: the same truth value for every voxel, one fp64 division per
// bisection step instead of one per voxel.  th = +inf (empty lobe): no k, no candidates.
__global__ __launch_bounds__(256) void chunk_prepare_kernel(PrepArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char prep_lds[];
    PrepX* xt = reinterpret_cast<PrepX*>(prep_lds);
    __shared__ PrepRow rt[PREP_MAX_ROWS];
    __shared__ int kcut_s;
    const int n = blockIdx.y;
    const ChunkRec r = a.table[n];
    const int nrows_all = a.Do * a.Ho;
    const int row0 = blockIdx.x * a.rows;
    const int nrows = nrows_all - row0 < a.rows ? nrows_all - row0 : a.rows;
    const bool empty = r.Di <= 0 || r.Hi <= 0 || r.Wi <= 0;
    if (!empty) {
        for (int x = threadIdx.x; x < a.Wo; x += 256) {
            const ItkAxis g = itk_axis(mul_rn((double)x, r.sx), r.Wi);
            xt[x].x0 = g.lo; xt[x].xn = g.inside ? g.nearest : -1; xt[x].tx = g.t;
        }
        if ((int)threadIdx.x < nrows) {
            const int row = row0 + threadIdx.x;
            PrepRow& p = rt[threadIdx.x];
            const ItkAxis gz = itk_axis(mul_rn((double)(row / a.Ho), r.sz), r.Di), gy = itk_axis(mul_rn((double)(row % a.Ho), r.sy), r.Hi);
            p.z0 = gz.lo; p.z1 = gz.hi; p.zn = gz.inside ? gz.nearest : -1; p.tz = gz.t;
            p.y0 = gy.lo; p.y1 = gy.hi; p.yn = gy.inside ? gy.nearest : -1; p.ty = gy.t;
        }
        if (threadIdx.x == 255) {
            int cut = 0x7fffffff;
            if (a.lesion_out) {
                const double th = a.th[n];
                const int span = a.pwmax - a.pwmin;
                int lo = 0, hi = span + 1;                         // smallest k in [0, span] with k / span > th; span + 1: none
                while (lo < hi) {
                    const int mid = lo + (hi - lo) / 2;
                    if (windowed_scan(a.pwmin + mid, a.pwmin, a.pwmax) > th) hi = mid; else lo = mid + 1;
                }
                cut = lo;
            }
            kcut_s = cut;
        }
    }
    __syncthreads();
    const int kcut = empty ? 0x7fffffff : kcut_s;
    const float range = (float)((double)a.wmax - (double)a.wmin);
    const int16_t* scan = a.scans + r.off;
    const uint8_t* lobe = a.lobes + r.off;
    const uint8_t* ves = a.vessels ? a.vessels + r.off : nullptr;
    const size_t HW = (size_t)r.Hi * r.Wi;

    // one output voxel: local row lr, column x -> image, lobe, lesion, vessel
    auto voxel = [&](int lr, int x, float& o_img, float& o_lobe, float& o_les, float& o_ves) {
#pragma clang fp contract(off)
        o_img = 0.f; o_lobe = 0.f; o_les = 0.f; o_ves = 0.f;
        if (empty) return;
        const PrepRow& p = rt[lr];
        const PrepX q = xt[x];
        if (p.zn < 0 || p.yn < 0 || q.xn < 0) return;              // beyond the source buffer: ITK's default value 0 everywhere
        const int x0 = q.x0, x1 = x0 + 1 <= r.Wi - 1 ? x0 + 1 : x0;
        const size_t r00 = (size_t)p.z0 * HW + (size_t)p.y0 * r.Wi, r01 = (size_t)p.z0 * HW + (size_t)p.y1 * r.Wi;
        const size_t r10 = (size_t)p.z1 * HW + (size_t)p.y0 * r.Wi, r11 = (size_t)p.z1 * HW + (size_t)p.y1 * r.Wi;
        const int16_t s000 = scan[r00 + x0], s001 = scan[r00 + x1], s010 = scan[r01 + x0], s011 = scan[r01 + x1];
        const int16_t s100 = scan[r10 + x0], s101 = scan[r10 + x1], s110 = scan[r11 + x0], s111 = scan[r11 + x1];
        auto w = [&](int16_t s) { return (double)window_f32(s, a.wmin, a.wmax, range); };
        const double v00 = lerp_rn(w(s000), w(s001), q.tx), v10 = lerp_rn(w(s010), w(s011), q.tx);
        const double v01 = lerp_rn(w(s100), w(s101), q.tx), v11 = lerp_rn(w(s110), w(s111), q.tx);
        o_img = (float)lerp_rn(lerp_rn(v00, v10, p.ty), lerp_rn(v01, v11, p.ty), p.tz);
        // the nearest voxel is a corner of the linear cell (c + 0.5 < size_in: base or base + 1, never past the clamp)
        const bool zu = p.zn != p.z0, yu = p.yn != p.y0, xu = q.xn != x0;
        const size_t near = (size_t)p.zn * HW + (size_t)p.yn * r.Wi + q.xn;
        const uint8_t l = lobe[near];
        o_lobe = (float)l;
        if (a.lesion_out) {
            const int16_t sa = xu ? s001 : s000, sb = xu ? s011 : s010, sc = xu ? s101 : s100, sd = xu ? s111 : s110;
            const int s = zu ? (yu ? sd : sc) : (yu ? sb : sa);
            const int c = s < a.pwmin ? a.pwmin : (s > a.pwmax ? a.pwmax : s);
            o_les = (l > 0 && c - a.pwmin >= kcut) ? 1.f : 0.f;
        }
        if (a.vessel_out) o_ves = (l > 0 && ves[near] > 0) ? 1.f : 0.f;
    };

    const size_t span0 = ((size_t)n * nrows_all + row0) * a.Wo;    // first element of the block's span in every output
    const size_t span1 = span0 + (size_t)nrows * a.Wo;
    const bool wide = ((((size_t)a.image) | ((size_t)a.lobe_out) | ((size_t)a.lesion_out) | ((size_t)a.vessel_out)) & 15) == 0;
    for (size_t q4 = (span0 >> 2) + threadIdx.x; (q4 << 2) < span1; q4 += 256) {
        const size_t e0 = q4 << 2;
        const size_t ea = e0 > span0 ? e0 : span0, eb = e0 + 4 < span1 ? e0 + 4 : span1;
        int lr = (int)((ea - span0) / a.Wo), x = (int)((ea - span0) % a.Wo);
        float vi[4], vl[4], vs[4], vv[4];
        for (size_t e = ea; e < eb; ++e) {
            const int k = (int)(e - e0);
            voxel(lr, x, vi[k], vl[k], vs[k], vv[k]);
            if (++x == a.Wo) { x = 0; ++lr; }
        }
        if (wide && ea == e0 && eb == e0 + 4) {
            *reinterpret_cast<float4*>(a.image + e0) = make_float4(vi[0], vi[1], vi[2], vi[3]);
            *reinterpret_cast<float4*>(a.lobe_out + e0) = make_float4(vl[0], vl[1], vl[2], vl[3]);
            if (a.lesion_out) *reinterpret_cast<float4*>(a.lesion_out + e0) = make_float4(vs[0], vs[1], vs[2], vs[3]);
            if (a.vessel_out) *reinterpret_cast<float4*>(a.vessel_out + e0) = make_float4(vv[0], vv[1], vv[2], vv[3]);
        } else {
            for (size_t e = ea; e < eb; ++e) {
                const int k = (int)(e - e0);
                a.image[e] = vi[k];
                a.lobe_out[e] = vl[k];
                if (a.lesion_out) a.lesion_out[e] = vs[k];
                if (a.vessel_out) a.vessel_out[e] = vv[k];
            }
        }
    }
}

}  // namespace dram

using namespace dram;

// hist: [N][256] uint64 (zeroed here).  scans / lobes: the packed buffers, 16-byte aligned bases; table: N ChunkRec on the device.
extern "C" int dram_chunk_hist256(const int16_t* scans, const uint8_t* lobes, const void* table, int N,
                                  unsigned long long* hist, int wmin, int wmax, void* stream) {
    DRAM_REQUIRE(scans && lobes && table && hist, "chunk_hist256: null pointer");
    DRAM_REQUIRE(N > 0 && N <= 65535, "chunk_hist256: N in 1..65535");
    DRAM_REQUIRE(wmax > wmin, "chunk_hist256: empty window");
    DRAM_REQUIRE(aligned16(scans) && aligned16(lobes), "chunk_hist256: the packed buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(hist, 0, (size_t)N * 256 * sizeof(unsigned long long), st);
    int per = 2048 / N;                            // ~2048 blocks in flight; a block past its chunk's end returns at once
    per = per < 8 ? 8 : (per > 512 ? 512 : per);
    hipLaunchKernelGGL(chunk_hist_kernel, dim3(per, N), dim3(256), 0, st, scans, lobes, (const ChunkRec*)table, hist, wmin, wmax);
    return check_launch("chunk_hist256");
}

extern "C" int dram_otsu256(const unsigned long long* hist, int N, double scaler, double* th, void* stream) {
    DRAM_REQUIRE(hist && th, "otsu256: null pointer");
    DRAM_REQUIRE(N > 0, "otsu256: N must be positive");
    DRAM_REQUIRE(scaler > 0.0, "otsu256: scaler must be positive");
    hipLaunchKernelGGL(otsu256_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, hist, scaler, th);
    return check_launch("otsu256");
}

extern "C" int dram_chunk_prepare(const int16_t* scans, const uint8_t* lobes, const uint8_t* vessels, const void* table,
                                  const double* th, int N, int Do, int Ho, int Wo, float wmin, float wmax, int pwmin, int pwmax,
                                  float* image, float* lobe_out, float* lesion_out, float* vessel_out, void* stream) {
    DRAM_REQUIRE(scans && lobes && table && image && lobe_out, "chunk_prepare: null pointer");
    DRAM_REQUIRE(N > 0 && N <= 65535, "chunk_prepare: N in 1..65535");
    DRAM_REQUIRE(Do > 0 && Ho > 0 && Wo > 0 && Wo <= PREP_MAX_WO && (int64_t)Do * Ho < 0x7fffffffLL,
                 "chunk_prepare: bad output size (Wo up to %d)", PREP_MAX_WO);
    DRAM_REQUIRE(wmax > wmin, "chunk_prepare: empty window");
    DRAM_REQUIRE(!lesion_out || (th && pwmax > pwmin), "chunk_prepare: the pseudo-lesion output needs thresholds and a window");
    DRAM_REQUIRE(!vessel_out || vessels, "chunk_prepare: the vessel output needs the vessel masks");
    PrepArgs a{scans, lobes, vessel_out ? vessels : nullptr, (const ChunkRec*)table, th, image, lobe_out, lesion_out, vessel_out,
               Do, Ho, Wo, 0, wmin, wmax, pwmin, pwmax};
    int rows = cdiv(2048, Wo);                     // ~2048 output voxels per output and block: 2 quads per thread
    rows = rows > PREP_MAX_ROWS ? PREP_MAX_ROWS : rows;
    a.rows = rows;
    hipLaunchKernelGGL(chunk_prepare_kernel, dim3(cdiv(Do * Ho, rows), N), dim3(256), (size_t)Wo * sizeof(PrepX),
                       (hipStream_t)stream, a);
    return check_launch("chunk_prepare");
}
