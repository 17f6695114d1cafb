// tri_oracle_main.cpp — TEST INFRASTRUCTURE: the oracle's own FeatureManager::triangulate and getDepthVector (oracle/sequence.cpp, included unchanged) on tables read
// from standard input, the depths written as hex floats. tests/test_feature_triangulate.py builds this with the oracle Makefile's flags against liboracle_vilf.so and
// compares tests/tri_reference.py with it to the bit.
//   input    n_tables, then per table: n_frames n_features init_depth, Ps [n_frames][3], Rs [n_frames][9], tic [3], ric [9], then per feature: start_frame n_obs depth
//            and n_obs points of 3. Numbers are hex floats (or nan / inf).
//   output   per table one line with the n_features depths after triangulate, one with n_used and getDepthVector.
#include "../oracle/sequence.cpp"
#include <cstdio>

static double rd() {
    double v = 0;
    if (std::scanf("%la", &v) != 1) { std::fprintf(stderr, "tri_oracle_main: bad input\n"); std::exit(2); }
    return v;
}
static int ri() {
    int v = 0;
    if (std::scanf("%d", &v) != 1) { std::fprintf(stderr, "tri_oracle_main: bad input\n"); std::exit(2); }
    return v;
}

int main() {
    const int n_tables = ri();
    for (int t = 0; t < n_tables; t++) {
        const int nf = ri(), n = ri();
        if (nf < 2 || nf > NFR || n < 0) { std::fprintf(stderr, "tri_oracle_main: bad sizes\n"); return 2; }
        FeatureManager fm;
        fm.init_depth = rd();
        V3 Ps[NFR]; M3 Rs[NFR];
        for (int k = 0; k < nf; k++) { double p[3]; for (double &v : p) v = rd(); Ps[k] = V3(p); }
        for (int k = 0; k < nf; k++) { double r[9]; for (double &v : r) v = rd(); Rs[k] = M3::from(r); }
        double tc[3], rc[9];
        for (double &v : tc) v = rd();
        for (double &v : rc) v = rd();
        for (int f = 0; f < n; f++) {
            const int start = ri(), nobs = ri();
            fm.feature.emplace_back(f, start, -1.0);
            FeaturePerId &it = fm.feature.back();
            it.estimated_depth = rd();
            for (int o = 0; o < nobs; o++) {
                FeaturePerFrame fp;
                double p[3]; for (double &v : p) v = rd();
                fp.point = V3(p); fp.uv[0] = fp.uv[1] = fp.velocity[0] = fp.velocity[1] = 0; fp.depth = -1; fp.cur_td = 0;
                it.feature_per_frame.push_back(fp);
            }
        }
        fm.triangulate(Ps, Rs, V3(tc), M3::from(rc));
        for (auto &it : fm.feature) std::printf("%a ", it.estimated_depth);
        std::printf("\n");
        std::vector<double> d = fm.getDepthVector();
        std::printf("%zu", d.size());
        for (double v : d) std::printf(" %a", v);
        std::printf("\n");
    }
    return 0;
}
