// tests/native/ks_raybatch.cpp -- TEST-ONLY host build of the ray walk (ks_obs.h: RayWalk) at several leaf batch sizes.
// For one reset pose it casts every (ray, mesh geom) pair the serial rangefinder() would cast - the same snapshot, ray_origin and
// ray_to_geom - and returns, per pair, the walk's result at LEAF_BATCH = 1 (the per-slot loops), 2 and 4 (the chunked loop) and the
// minimum of ray_tri over ALL triangles of the mesh, and counts what the walks met: leaf sizes and leaf children per node visit.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../kinovagrasping_amd/csrc/ks_env.h"
#include "../../kinovagrasping_amd/csrc/ks_model_host.h"

using namespace ks;

template <typename T> struct SnapPut {
    T* s;
    void operator()(int k, T v) const { s[k] = v; }
};

// leaf children of `node` that a step() with pruning distance tmax would test: sizes into size_hist[1..7] (size_hist[0]: the leaf among them
// that ends the triangle table), their number into kids_hist[0..4]
static void count_node(const float* wnode, int node, int ntri, const float* lp, const float* inv, const bool* par, float tmax, long* size_hist, long* kids_hist) {
    const float* w = wnode + 32 * (long)node;
    int kids = 0;
    for (int k = 0; k < 4; k++) {
        const int id = float_bits(w[24 + k]);
        if (id == RAY_EMPTY || id >= 0) continue;
        if (bvh_box_entry_inv(w + 6 * k, lp, inv, par, tmax) < 0) continue;
        size_hist[(-id - 1) & 7]++;
        if (((-id - 1) >> 3) + ((-id - 1) & 7) == ntri) size_hist[0]++;
        kids++;
    }
    kids_hist[kids]++;
}

// one walk through the tables of a mesh (tri [ntri][9], wnode [wide nodes][32]; size: the half-extents of its bounding box about the origin)
template <int B> static float walk(const float* tri, const float* wnode, int ntri, const float* size, const float* lp, const float* lv, long* size_hist, long* kids_hist) {
    RayWalk<float, OwnBound, LocalStack<float>, B> w;
    if (!w.start(tri, wnode, size, lp, lv, OwnBound(), LocalStack<float>())) return -1.0f;
    for (;;) {
        if (size_hist) count_node(w.wnode, w.node, ntri, w.lp, w.inv, w.par, w.bound(w.best), size_hist, kids_hist);
        if (!w.step()) break;
    }
    return w.best;
}

static float exhaustive(const float* tri, int ntri, const float* size, const float* lp, const float* lv) {
    const float lo[3] = {-size[0], -size[1], -size[2]}, hi[3] = {size[0], size[1], size[2]};
    if (!ray_box(lp, lv, lo, hi, Lim<float>::big)) return -1.0f;              // the walk's own first test (mj_rayMesh's)
    float best = -1.0f;
    for (int i = 0; i < ntri; i++) {
        const float tt = ray_tri(&tri[9 * (long)i], lp, lv);
        if (tt >= 0 && (best < 0 || tt < best)) best = tt;
    }
    return best;
}

// o [4]: the walks at LEAF_BATCH 1, 2, 4 and the exhaustive minimum; the histograms from the LEAF_BATCH = 1 walk
static void cast_all(const float* tri, const float* wnode, int ntri, const float* size, const float* lp, const float* lv, float* o, long* size_hist, long* kids_hist) {
    o[0] = walk<1>(tri, wnode, ntri, size, lp, lv, size_hist, kids_hist);
    o[1] = walk<2>(tri, wnode, ntri, size, lp, lv, nullptr, nullptr);
    o[2] = walk<4>(tri, wnode, ntri, size, lp, lv, nullptr, nullptr);
    o[3] = exhaustive(tri, ntri, size, lp, lv);
}

extern "C" {
void* rb_create(const void* blob, size_t n) {
    HostModel<float>* h = new HostModel<float>();
    if (!parse_model<float>(blob, n, *h)) {
        std::fprintf(stderr, "rb_create: %s\n", h->error.c_str());
        delete h;
        return nullptr;
    }
    return h;
}
void rb_destroy(void* h) { delete (HostModel<float>*)h; }
int rb_ngeom(void* h) { return ((HostModel<float>*)h)->m.ngeom; }
int rb_geom_mesh(void* h, int g) { return ((HostModel<float>*)h)->m.geom_mesh[g]; }
// a mesh's whole hierarchy, not a walk: leaves by size [8], wide nodes by their number of leaf children [5], triangles
void rb_mesh_shape(void* h, int mesh, long* size_table, long* kids_table, int* ntri) {
    const Model<float>& m = ((HostModel<float>*)h)->m;
    *ntri = m.mesh_ntri[mesh];
    const size_t nwide = ((HostModel<float>*)h)->bvh_box[mesh].size() / 32;
    for (size_t nd = 0; nd < nwide; nd++) {
        int kids = 0;
        for (int k = 0; k < 4; k++) {
            const int id = float_bits(m.mesh_bvh_box[mesh][32 * nd + 24 + k]);
            if (id == RAY_EMPTY || id >= 0) continue;
            kids++;
            size_table[(-id - 1) & 7]++;
        }
        kids_table[kids]++;
    }
}
// out [17][ngeom][4]: walks at LEAF_BATCH 1, 2, 4 and the exhaustive minimum (-2 where rangefinder() casts nothing: geom 0, the ray's own body);
// size_hist [ngeom][8] ([0]: visits of the table's last leaf), kids_hist [ngeom][5]: accumulated over the LEAF_BATCH = 1 walks, by geom
void rb_cast(void* h, const double* qpos0, const double* hq, float* out, long* size_hist, long* kids_hist) {
    const Model<float>& m = ((HostModel<float>*)h)->m;
    std::vector<float> scrbuf(SCR_TOTAL, 0.f), snapbuf(SNAP_TOTAL, 0.f);
    Scratch<float> scr{scrbuf.data(), 1};
    { float mass, mu; nominal_env_params(m, mass, mu); scr(SCR_ENVP) = mass; scr(SCR_ENVP + 1) = mu; }
    LaneState<float> st;
    float q4[4], q0[NQ];
    for (int i = 0; i < NQ; i++) q0[i] = st.qpos[i] = (float)qpos0[i];
    for (int i = 0; i < NV; i++) st.qvel[i] = st.warm[i] = 0.f;
    for (int i = 0; i < 4; i++) q4[i] = (float)hq[i];
    lane_reset(m, st, q4, q0, scr, SnapPut<float>{snapbuf.data()});
    Col<float> snap{snapbuf.data(), 1};
    for (int r = 0; r < NRAY; r++) {
        float pnt[3], vec[3];
        const int sb = ray_origin(m, snap, r, pnt, vec);
        for (int g = 0; g < m.ngeom; g++) {
            float* o = out + ((long)r * m.ngeom + g) * 4;
            if (g == 0 || m.geom_body[g] == sb) { o[0] = o[1] = o[2] = o[3] = -2.0f; continue; }
            float lp[3], lv[3];
            ray_to_geom(m, snap, g, pnt, vec, lp, lv);
            const int mesh = m.geom_mesh[g];
            cast_all(m.mesh_tri[mesh], m.mesh_bvh_box[mesh], m.mesh_ntri[mesh], m.geom_size[g], lp, lv, o, size_hist + 8 * g, kids_hist + 5 * g);
        }
    }
}
// n rays given in the frame of geom g (lp, lv [n][3]); out [n][4], size_hist [8], kids_hist [5] as above
void rb_cast_local(void* h, int g, int n, const float* lp, const float* lv, float* out, long* size_hist, long* kids_hist) {
    const Model<float>& m = ((HostModel<float>*)h)->m;
    const int mesh = m.geom_mesh[g];
    for (int i = 0; i < n; i++)
        cast_all(m.mesh_tri[mesh], m.mesh_bvh_box[mesh], m.mesh_ntri[mesh], m.geom_size[g], lp + 3 * i, lv + 3 * i, out + 4 * i, size_hist, kids_hist);
}
// n rays (lp, lv [n][3], in the mesh's frame) through tables of the caller's own making - exactly ntri * 9 and nwide * 32 floats, copied into
// heap blocks of that size, so that a read beyond them is an AddressSanitizer finding; out [n][4], size_hist [8], kids_hist [5] as above
void rb_cast_tables(const float* tri, int ntri, const float* wnode, int nwide, const float* size, int n, const float* lp, const float* lv, float* out,
                    long* size_hist, long* kids_hist) {
    const std::vector<float> t(tri, tri + 9 * (size_t)ntri), w(wnode, wnode + 32 * (size_t)nwide);
    for (int i = 0; i < n; i++) cast_all(t.data(), w.data(), ntri, size, lp + 3 * i, lv + 3 * i, out + 4 * i, size_hist, kids_hist);
}
}
