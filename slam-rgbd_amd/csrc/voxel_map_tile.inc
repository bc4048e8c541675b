// voxel_map_tile.inc -- the body of k_map_integrate and of k_map_update
// (voxel_map.hip): one 2048-pixel tile of one frame into the map or, with
// kRemove, out of it.  The LDS table sums a tile's runs the same way in both;
// only its flush (and the direct path) adds or subtracts.
//
// Included into both kernels, not called: as an inlined device function the
// same statements compile k_map_integrate to other code than it had before
// removal existed (its pointers travel as generic ones, and operand order and
// register allocation follow; profiles/mapmove/isa_identical.txt), and the
// adding kernel is to stay the kernel that was measured.
//
// Expects in scope: the template parameters kVec, kLds, kRgb; constexpr bool
// kRemove; the kernel's arguments depth, rgb, W, N, K, T_world, vpm,
// max_depth, t.
    __shared__ __align__(8) unsigned char lds_raw[kLds ? sizeof(LdsTable) : 8];
    LdsTable* lt = reinterpret_cast<LdsTable*>(lds_raw);   // unused without kLds
    if (kLds) {
        for (int s = threadIdx.x; s < kLdsSlots; s += kMapThreads) {
            lt->keys[s] = kEmpty;
#pragma unroll
            for (int j = 0; j < 7; ++j) lt->vals[j][s] = 0;
        }
        __syncthreads();
    }
    const int f = blockIdx.y, tile = blockIdx.x;
    const int i = (tile * kMapThreads + threadIdx.x) * kMapPx;
    int dd[kMapPx];
    youth_cloud::load_depth<kVec, kMapPx>(depth + (size_t)f * N, i, N, dd);
    unsigned char cc[kMapPx * 3];
    if (kRgb) {
        youth_cloud::load_rgb<kVec, kMapPx>(rgb + ((size_t)f * N + i) * 3, i, N, cc);
    } else {
#pragma unroll
        for (int k = 0; k < kMapPx * 3; ++k) cc[k] = 0;
    }
    // frame f's camera -> world pose, or the identity: one path, the same fma chains
    float Tw[12] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    if (T_world) {
#pragma unroll
        for (int q = 0; q < 12; ++q) Tw[q] = T_world[(size_t)f * 12 + q];
    }
    Tally n;
    Acc cur;
    bool have = false;
    // (u, v) of pixel i; a thread's pixels may wrap rows (any W >= 1)
    int v = i / W;
    int u = i - v * W;
#pragma unroll
    for (int k = 0; k < kMapPx; ++k) {
        const int d = dd[k];
        if (d > 0 && (max_depth == 0 || d <= max_depth)) {
            float x, y, z;
            youth_cloud::camera_point(d, u, v, K, x, y, z);
            const float X = youth_cloud::world_axis(Tw, x, y, z);
            const float Y = youth_cloud::world_axis(Tw + 4, x, y, z);
            const float Z = youth_cloud::world_axis(Tw + 8, x, y, z);
            uint32_t cx, cy, cz, qx, qy, qz;
            const bool in = axis_key(X, vpm, cx, qx) && axis_key(Y, vpm, cy, qy) &&
                            axis_key(Z, vpm, cz, qz);
            if (in) {
                const unsigned long long key =
                    ((unsigned long long)cz << 42) | ((unsigned long long)cy << 21) | cx;
                if (have && key != cur.key) {
                    emit_run<kLds, kRgb, kRemove>(t, lt, cur, n);
                    have = false;
                }
                if (!have) {
                    cur.key = key;
                    cur.cnt = 0;
#pragma unroll
                    for (int j = 0; j < 3; ++j) cur.q[j] = cur.c[j] = 0;
                    have = true;
                }
                ++cur.cnt;
                cur.q[0] += qx;
                cur.q[1] += qy;
                cur.q[2] += qz;
#pragma unroll
                for (int j = 0; j < 3; ++j) cur.c[j] += cc[3 * k + j];
            } else if (!kRemove) {
                ++n.out_of_range;
            }
        }
        ++u;
        while (u >= W) {
            u -= W;
            ++v;
        }
    }
    if (have) emit_run<kLds, kRgb, kRemove>(t, lt, cur, n);
    if (kLds) {
        __syncthreads();
        for (int s = threadIdx.x; s < kLdsSlots; s += kMapThreads) {
            Acc a;
            a.key = lt->keys[s];
            if (a.key == kEmpty) continue;
            a.cnt = lt->vals[0][s];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                a.q[j] = lt->vals[1 + j][s];
                a.c[j] = lt->vals[4 + j][s];
            }
            global_add<kRgb, kRemove>(t, a, n);
        }
    }
    // the counters: one add per wave and counter that has something to add
    if (kRemove) {
        const uint32_t sums[3] = {wave_sum_u32(n.integrated), wave_sum_u32(n.dropped),
                                  wave_sum_u32(n.occupied)};
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (sums[j]) atomicAdd(&t.stats[kStRemoved + j], (unsigned long long)sums[j]);
        }
    } else {
        const uint32_t sums[5] = {wave_sum_u32(n.integrated), wave_sum_u32(n.out_of_range),
                                  wave_sum_u32(n.dropped), wave_sum_u32(n.occupied),
                                  wave_sum_u32(n.direct)};
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int j = 0; j < 5; ++j)
                if (sums[j]) atomicAdd(&t.stats[j], (unsigned long long)sums[j]);
        }
    }
