// A view's three-panel visualisation (include/suo_hip.h states every rule): viz_splat_kernel projects the overlay objects' mesh points into an owner plane,
// viz_compose_kernel writes the [H][3 W][3] canvas, one thread per output pixel.  Integers, fp64 and fp32 with + - x / only; the build's -ffp-contract=off
// keeps every product and sum as written, which is what makes the result equal to the numpy statement of the rules byte for byte.
#include <math.h>

#include <mutex>

#include "viz.h"

namespace suo {

// The stamp weights of csrc/misc.hip (c_prior_w: the same expression on the same host libm; a __constant__ belongs to its translation unit, and that file is
// not changed for this) and the 41 keypoint colours, packed b | g << 8 | r << 16.
constexpr int VZ_HALF = 45, VZ_SIZE = 2 * VZ_HALF + 1;
__constant__ double c_viz_w[VZ_SIZE];
__constant__ int c_viz_kp_colour[VIZ_KP_COLOURS];

int viz_upload_tables(const uint8_t* kp_bgr) {
    static int rc = -1;
    static std::once_flag once;
    std::call_once(once, [kp_bgr] {
        double w[VZ_SIZE];
        const double sigma = 0.3 * ((VZ_SIZE - 1) * 0.5 - 1) + 0.8;
        for (int i = 0; i < VZ_SIZE; ++i) {
            const double d = (double)i - (VZ_SIZE - 1) / 2;
            w[i] = exp(-(d * d) / (2 * sigma * sigma)) * ((i == 0 || i == VZ_SIZE - 1) ? 2.0 : 1.0);
        }
        int col[VIZ_KP_COLOURS];
        for (int k = 0; k < VIZ_KP_COLOURS; ++k) col[k] = kp_bgr[3 * k] | kp_bgr[3 * k + 1] << 8 | kp_bgr[3 * k + 2] << 16;
        rc = (hipMemcpyToSymbol(HIP_SYMBOL(c_viz_w), w, sizeof(w)) == hipSuccess &&
              hipMemcpyToSymbol(HIP_SYMBOL(c_viz_kp_colour), col, sizeof(col)) == hipSuccess) ? SUO_OK : SUO_ERR_HIP;
    });
    if (rc) suo_set_error("suo_viz_create: table upload failed");
    return rc;
}

// ---- right panel, first half: who owns a pixel ------------------------------------------------------------------------------------------------------------
// One thread per (overlay object, mesh point): blockIdx.y is the object's rank in paint order.  atomicMax(rank + 1) makes "later objects overwrite earlier ones"
// independent of the order in which the points arrive.
__global__ __launch_bounds__(256) void viz_splat_kernel(VizArgs a) {
    const VizOverlay& ov = a.ov[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ov.count) return;
    const float* p = a.pts + ((size_t)ov.first + i) * 3;
    const double x = p[0], y = p[1], z = p[2];
    const double* T = ov.T;
    const double* K = ov.K;
    const double X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    const double Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    const double Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    const double wa = (K[0] * X + K[1] * Y) + K[2] * Z;
    const double wb = (K[3] * X + K[4] * Y) + K[5] * Z;
    const double wc = (K[6] * X + K[7] * Y) + K[8] * Z;
    const double u = wa / wc, v = wb / wc;
    if (!isfinite(u) || !isfinite(v)) return;
    const double uh = u + 0.5, vh = v + 0.5;
    if (fabs(uh) >= 2147483648.0 || fabs(vh) >= 2147483648.0) return;
    const int px = (int)uh, py = (int)vh;                          // toward zero
    if (px < 0 || py < 0 || px >= a.W || py >= a.H) return;
    atomicMax(&a.owner[(size_t)py * a.W + px], (int)blockIdx.y + 1);
}

// ---- the canvas ---------------------------------------------------------------------------------------------------------------------------------------------
// A workgroup is a 64 x 4 pixel tile of ONE panel (blockIdx.z), a wave one row of it: the panel's primitive table is staged in LDS in chunks, and every loop
// over it is the same in all lanes -- a primitive whose extent misses the tile is rejected before any lane looks at its own pixel.
constexpr int VZ_TX = 64, VZ_TY = 4, VZ_CHUNK = 128;               // 128 VizKp = 6 KiB; 128 stamps = 4 KiB; 64 boxes = 1.25 KiB

__device__ __forceinline__ bool viz_in_ellipse(double xr, double yr, int a, int b) {
    const double ab = (double)a * (double)b, t1 = xr * (double)b, t2 = yr * (double)a;
    return t1 * t1 + t2 * t2 <= ab * ab;
}

__global__ __launch_bounds__(256) void viz_compose_kernel(VizArgs a) {
    __shared__ int s_tab[VZ_CHUNK * (int)(sizeof(VizKp) / sizeof(int))];
    const int panel = blockIdx.z, tid = threadIdx.x;
    const int tiles_x = (a.W + VZ_TX - 1) / VZ_TX;                 // (tiles linearised on x: a grid's y extent stops at 65535)
    const int tx0 = (int)(blockIdx.x % tiles_x) * VZ_TX, ty0 = (int)(blockIdx.x / tiles_x) * VZ_TY;
    const int x = tx0 + (tid & (VZ_TX - 1)), y = ty0 + tid / VZ_TX;
    const bool live = x < a.W && y < a.H;                          // (no early return: the staging below has barriers)
    const long long tx1 = tx0 + VZ_TX - 1, ty1 = ty0 + VZ_TY - 1;
    int col = 0;
    if (live) {
        const uint8_t* f = a.frame + ((size_t)y * a.W + x) * 3;
        col = f[0] | f[1] << 8 | f[2] << 16;
    }

    if (panel == 2) {                                              // right: the 3 x 3 maximum of the owner plane
        if (live && a.n_ov > 0) {
            int m = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx, yy = y + dy;
                    if (xx >= 0 && yy >= 0 && xx < a.W && yy < a.H) m = max(m, a.owner[(size_t)yy * a.W + xx]);
                }
            if (m > 0) col = a.ov[m - 1].colour;
        }
    } else if (panel == 1) {                                       // centre: keypoints, the last hit wins
        for (int base = 0; base < a.n_kp; base += VZ_CHUNK) {
            const int n = min(VZ_CHUNK, a.n_kp - base), words = n * (int)(sizeof(VizKp) / sizeof(int));
            __syncthreads();
            for (int i = tid; i < words; i += 256) s_tab[i] = ((const int*)(a.kp + base))[i];
            __syncthreads();
            const VizKp* kp = (const VizKp*)s_tab;
            for (int j = 0; j < n; ++j) {
                const VizKp p = kp[j];
                long long R = max(p.r_outer, p.r_inner);
                if (p.has_ellipse) R = max(R, (long long)max(p.A, p.B) + 1);
                if (p.x + R < tx0 || p.x - R > tx1 || p.y + R < ty0 || p.y - R > ty1) continue;
                if (!live) continue;
                const long long dx = (long long)x - p.x, dy = (long long)y - p.y, d2 = dx * dx + dy * dy;
                if (d2 <= (long long)p.r_outer * p.r_outer) col = 0;
                if (d2 <= (long long)p.r_inner * p.r_inner) col = p.colour;
                if (p.has_ellipse) {
                    const double fx = (double)dx, fy = (double)dy;
                    const double xr = fx * p.c + fy * p.s, yr = -fx * p.s + fy * p.c;
                    if (viz_in_ellipse(xr, yr, p.A + 1, p.B + 1) && !(p.A >= 2 && p.B >= 2 && viz_in_ellipse(xr, yr, p.A - 1, p.B - 1))) col = p.colour;
                }
            }
        }
    } else {                                                       // left: boxes, then the prior heat blended in
        __syncthreads();
        for (int i = tid; i < a.n_box * VIZ_BOX_INTS; i += 256) s_tab[i] = a.box[i];
        __syncthreads();
        for (int j = 0; j < a.n_box; ++j) {
            const int* q = s_tab + j * VIZ_BOX_INTS;
            const long long x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
            if (x2 + 1 < tx0 || x1 - 1 > tx1 || y2 + 1 < ty0 || y1 - 1 > ty1) continue;
            const bool outer = x >= x1 - 1 && x <= x2 + 1 && y >= y1 - 1 && y <= y2 + 1;
            const bool inner = x >= x1 + 2 && x <= x2 - 2 && y >= y1 + 2 && y <= y2 - 2;
            if (live && outer && !inner) col = q[4];
        }
        // channels outside, a channel's stamps inside: the stamps arrive sorted by channel, so one pass over them closes a channel whenever the next begins
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
        float s = 0.f;
        int cur = -1;
        auto close = [&] {
            if (cur < 0) return;
            const double sc = (double)fminf(fmaxf(s, 0.f), 1.f);
            const int kc = c_viz_kp_colour[cur];
            acc0 += sc * (double)(kc & 255); acc1 += sc * (double)((kc >> 8) & 255); acc2 += sc * (double)((kc >> 16) & 255);
        };
        for (int base = 0; base < a.n_stamp; base += VZ_CHUNK) {
            const int n = min(VZ_CHUNK, a.n_stamp - base), words = n * VIZ_STAMP_INTS;
            __syncthreads();
            for (int i = tid; i < words; i += 256) s_tab[i] = a.stamp[(size_t)base * VIZ_STAMP_INTS + i];
            __syncthreads();
            for (int j = 0; j < n; ++j) {
                const int* q = s_tab + j * VIZ_STAMP_INTS;
                if (q[0] != cur) { close(); cur = q[0]; s = 0.f; }
                const long long ulx = q[1], uly = q[2];
                const long long lx = max(ulx, (long long)q[3]), hx = min(ulx + 2 * VZ_HALF, (long long)q[4]);      // [lx, hx) x [ly, hy)
                const long long ly = max(uly, (long long)q[5]), hy = min(uly + 2 * VZ_HALF, (long long)q[6]);
                if (hx <= tx0 || lx > tx1 || hy <= ty0 || ly > ty1) continue;
                if (live && x >= lx && x < hx && y >= ly && y < hy) s += (float)(c_viz_w[y - uly] * c_viz_w[x - ulx]);
            }
        }
        close();
        if (live) {
            int pc[3];
            const double acc[3] = {acc0, acc1, acc2};
            for (int c = 0; c < 3; ++c) pc[c] = (int)fmin(fmax(acc[c], 0.0), 255.0);
            const int gray = (1868 * pc[0] + 9617 * pc[1] + 4899 * pc[2] + 8192) >> 14;
            const float p = (float)gray / 255.f, q = 1.f - p;
            int o = 0;
            for (int c = 0; c < 3; ++c) o |= (int)(q * (float)((col >> (8 * c)) & 255) + p * (float)pc[c]) << (8 * c);
            col = o;
        }
    }
    if (live) {
        uint8_t* o = a.out + (((size_t)y * 3 + panel) * a.W + x) * 3;
        o[0] = (uint8_t)(col & 255); o[1] = (uint8_t)((col >> 8) & 255); o[2] = (uint8_t)((col >> 16) & 255);
    }
}

int viz_enqueue(const VizArgs& a, hipStream_t s) {
    if (a.n_ov > 0 && a.max_pts > 0) hipLaunchKernelGGL(viz_splat_kernel, dim3((a.max_pts + 255) / 256, a.n_ov), dim3(256), 0, s, a);
    hipLaunchKernelGGL(viz_compose_kernel, dim3(((a.W + VZ_TX - 1) / VZ_TX) * ((a.H + VZ_TY - 1) / VZ_TY), 1, 3), dim3(256), 0, s, a);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

}  // namespace suo
