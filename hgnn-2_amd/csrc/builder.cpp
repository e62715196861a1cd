// Native operator builder and sparse batcher (host C++).
//
// graph_operators (reference functions/operators.py:11-83) builds, per graph,
//   W  (N, N, J+2)  = [I, diag(sum_j A_ij), A, A^2, A^4, ...]
//   WL (M, M, J+2)  = [I, diag(sum AL), AL, AL^2, ...]   M = nnz(A) incl. the diagonal (Q2)
//   Pm, Pd (N, M)   incidence of the M edge slots
// with an O(N^2 + M^2) Python loop (24 ms per QM9-shape graph, 1.66 s per SBM-50
// graph), and prepare_batch (functions/batching.py:77-185) pads every
// graph to dense (bs, Nmax, Nmax, J+2) / (bs, Emax, Emax, J+2) / (bs, Nmax, Emax)
// tensors that the executor then re-extracts into row lists on the device.
//
// Here the same operators are built in C++:
//  * hgnn_graph_operators: the dense per-graph tensors of the reference (the
//    drop-in functions.operators.graph_operators calls it);
//  * hgnn_csr_batch_plan / _build: a whole batch straight into the executor's
//    packed sparse layout (node / edge-slot rows of all graphs back to back, one
//    entry per (row, col) of the union of the J+2 slices, ascending columns --
//    the order the device extraction produces, so both paths sum identically),
//    plus packed X / XL and the batch offsets: one host image, one H2D copy of a
//    few MB instead of the ~44 MB of dense operators per bs = 512 batch.
//
// Bit-exactness.  The edge-slot construction reproduces the reference's quirk
// (Q1: `e` advances once per undirected bond while two columns are written, so
// column k holds reverse(bond k-1) overlaid by forward(bond k), columns past B
// are "phantom" slots with edge (0, 0, 0)), and AL is evaluated on the float edge
// table exactly as the reference's loop does (operators.py:68-71).  Degrees, row
// sums and matrix powers are accumulated in double and rounded once: for the
// operator values of this domain (bond orders 1/1.5/2/3, 0/1 adjacency) every
// partial sum is exactly representable in fp32, so the result equals torch's fp32
// reduction bit for bit in any summation order.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/hgnn_amd.h"

namespace {

struct Row {  // == hgnn::RowInfo (csrc/common.h)
    int32_t start;
    int32_t count;
};

enum { K_W = 0, K_WT = 1, K_WL = 2, K_WLT = 3, K_PN = 4, K_PE = 5, K_N = 6 };

struct Edge {
    float src, tgt, w;
};

// The reference's edge table and incidence (operators.py:36-66), Q1 included.
// Returns false where the reference raises IndexError (a bond writes column M).
bool edge_slots(int n, const float* A, int m, std::vector<Edge>& edges, std::vector<float>* Pm,
                std::vector<float>* Pd) {
    edges.assign(m, Edge{0.f, 0.f, 0.f});
    if (Pm) Pm->assign((size_t)n * m, 0.f);
    if (Pd) Pd->assign((size_t)n * m, 0.f);
    int e = 0;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const float w = A[(size_t)i * n + j];
            if (w == 0.f) continue;
            if (e + 1 >= m) return false;
            // forward slot e, then the reverse slot e + 1 (overwritten by the next bond's forward)
            edges[e] = Edge{(float)i, (float)j, w};
            if (Pm) {
                (*Pm)[(size_t)i * m + e] = 1.f;
                (*Pm)[(size_t)j * m + e] = 1.f;
                (*Pd)[(size_t)i * m + e] = 1.f;
                (*Pd)[(size_t)j * m + e] = -1.f;
            }
            ++e;
            edges[e] = Edge{(float)j, (float)i, w};
            if (Pm) {
                (*Pm)[(size_t)j * m + e] = 1.f;
                (*Pm)[(size_t)i * m + e] = 1.f;
                (*Pd)[(size_t)j * m + e] = 1.f;
                (*Pd)[(size_t)i * m + e] = -1.f;
            }
        }
    return true;
}

int nnz_of(int n, const float* A) {
    int c = 0;
    for (size_t i = 0; i < (size_t)n * n; ++i) c += A[i] != 0.f;
    return c;
}

// Sparse matrix with sorted rows (value per column), used for A, AL and their powers.
struct Sp {
    int n = 0;
    std::vector<std::vector<std::pair<int, double>>> rows;
};

Sp square(const Sp& s) {
    Sp r;
    r.n = s.n;
    r.rows.resize(s.n);
    std::vector<double> acc(s.n, 0.0);
    std::vector<char> hit(s.n, 0);
    std::vector<int> cols;
    for (int i = 0; i < s.n; ++i) {
        cols.clear();
        for (auto& [k, a] : s.rows[i])
            for (auto& [j, b] : s.rows[k]) {
                if (!hit[j]) {
                    hit[j] = 1;
                    cols.push_back(j);
                }
                acc[j] += a * b;
            }
        std::sort(cols.begin(), cols.end());
        for (int j : cols) {
            // torch.matmul keeps explicit zeros out of nothing: a zero sum stays 0
            if (acc[j] != 0.0) r.rows[i].push_back({j, (double)(float)acc[j]});
            acc[j] = 0.0;
            hit[j] = 0;
        }
    }
    return r;
}

// All J+2 slices of one operator family as a sparse union: per row, ascending
// columns, jt coefficients per entry.
struct Ops {
    int n = 0, jt = 0;
    std::vector<std::vector<int>> cols;
    std::vector<std::vector<float>> vals;  // [row][entry * jt + j]
};

Ops slices(const Sp& base, int jt) {
    // slice 0 = I, 1 = diag(row sums of base), 2 = base, 3.. = base^(2^k)
    Ops o;
    o.n = base.n;
    o.jt = jt;
    std::vector<Sp> pw{base};
    for (int j = 3; j < jt; ++j) pw.push_back(square(pw.back()));
    o.cols.resize(base.n);
    o.vals.resize(base.n);
    for (int r = 0; r < base.n; ++r) {
        double deg = 0.0;
        for (auto& [c, v] : base.rows[r]) deg += v;
        // merge the columns of every slice (all sorted)
        std::vector<int> cs{r};
        for (const Sp& p : pw)
            for (auto& [c, v] : p.rows[r]) cs.push_back(c);
        std::sort(cs.begin(), cs.end());
        cs.erase(std::unique(cs.begin(), cs.end()), cs.end());
        std::vector<float> vs(cs.size() * jt, 0.f);
        for (size_t e = 0; e < cs.size(); ++e) {
            if (cs[e] == r) {
                vs[e * jt + 0] = 1.f;
                vs[e * jt + 1] = (float)deg;
            }
        }
        for (size_t p = 0; p < pw.size(); ++p)
            for (auto& [c, v] : pw[p].rows[r]) {
                const size_t e = std::lower_bound(cs.begin(), cs.end(), c) - cs.begin();
                vs[e * jt + 2 + p] = (float)v;
            }
        // drop entries whose every slice is zero (e.g. an isolated node's diagonal keeps I = 1, so none here)
        o.cols[r] = std::move(cs);
        o.vals[r] = std::move(vs);
    }
    return o;
}

Sp adjacency(int n, const float* A) {
    Sp s;
    s.n = n;
    s.rows.resize(n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const float v = A[(size_t)i * n + j];
            if (v != 0.f) s.rows[i].push_back({j, (double)v});
        }
    return s;
}

// AL[m1, m2] = w(m2) if tgt(m1) == src(m2) and src(m1) != tgt(m2) (operators.py:68-71)
Sp line_graph(const std::vector<Edge>& edges) {
    const int m = (int)edges.size();
    Sp s;
    s.n = m;
    s.rows.resize(m);
    // bucket slots by src (integers stored as floats; phantom slots have src 0)
    int nn = 0;
    for (const Edge& e : edges) nn = std::max(nn, (int)e.src + 1);
    std::vector<std::vector<int>> by_src(nn);
    for (int k = 0; k < m; ++k) by_src[(int)edges[k].src].push_back(k);
    for (int a = 0; a < m; ++a) {
        const int t = (int)edges[a].tgt;
        if (t >= nn) continue;
        for (int b : by_src[t])
            if (edges[a].src != edges[b].tgt) {
                // where(cond, w, 0): a zero weight (phantom column) contributes an explicit 0 -> no entry
                if (edges[b].w != 0.f) s.rows[a].push_back({b, (double)edges[b].w});
            }
    }
    return s;
}

Ops transpose(const Ops& o) {
    Ops t;
    t.n = o.n;
    t.jt = o.jt;
    t.cols.resize(o.n);
    t.vals.resize(o.n);
    for (int r = 0; r < o.n; ++r)
        for (size_t e = 0; e < o.cols[r].size(); ++e) {
            const int c = o.cols[r][e];
            t.cols[c].push_back(r);
            for (int j = 0; j < o.jt; ++j) t.vals[c].push_back(o.vals[r][e * o.jt + j]);
        }
    return t;  // rows visited in ascending order -> columns of t ascending
}

struct GraphBuild {
    int n = 0, m = 0;
    Ops W, WT, WL, WLT;
    // incidence rows: node n -> (slot, pm, pd); slot m -> (node, pm, pd)
    std::vector<std::vector<std::pair<int, std::pair<float, float>>>> pn, pe;
    std::vector<float> xl;  // DL diagonal (functions/batching.py:171)
};

int build_graph(int n, const float* A, int jt, bool dual, GraphBuild& g) {
    g.n = n;
    const Sp a = adjacency(n, A);
    g.W = slices(a, jt);
    g.WT = transpose(g.W);
    if (!dual) return HGNN_OK;
    g.m = nnz_of(n, A);
    std::vector<Edge> edges;
    std::vector<float> Pm, Pd;
    if (!edge_slots(n, A, g.m, edges, &Pm, &Pd)) return HGNN_ERR_INDEX;
    const Sp al = line_graph(edges);
    g.WL = slices(al, jt);
    g.WLT = transpose(g.WL);
    g.xl.resize(g.m);
    for (int r = 0; r < g.m; ++r) {
        double s = 0.0;
        for (auto& [c, v] : al.rows[r]) s += v;
        g.xl[r] = (float)s;
    }
    g.pn.assign(n, {});
    g.pe.assign(g.m, {});
    for (int i = 0; i < n; ++i)
        for (int e = 0; e < g.m; ++e) {
            const float pm = Pm[(size_t)i * g.m + e], pd = Pd[(size_t)i * g.m + e];
            if (pm != 0.f || pd != 0.f) g.pn[i].push_back({e, {pm, pd}});
        }
    for (int e = 0; e < g.m; ++e)
        for (int i = 0; i < n; ++i) {
            const float pm = Pm[(size_t)i * g.m + e], pd = Pd[(size_t)i * g.m + e];
            if (pm != 0.f || pd != 0.f) g.pe[e].push_back({i, {pm, pd}});
        }
    return HGNN_OK;
}

int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

}  // namespace

namespace hgnn {
// The image's field order and byte offsets from the counts (bs, f_in, dual, stride_w, nodes, edges and nnz
// filled in): the one place they are formed, for the host batcher (csr_batch) and for the device batcher's
// layout (hgnn_csr_layout_from_counts).
void csr_layout_offsets(hgnn_csr_layout& L) {
    const int bs = L.bs, sw = L.stride_w;
    const int64_t rows_of[K_N] = {L.nodes, L.nodes, L.edges, L.edges, L.nodes, L.edges};
    const int stride_of[K_N] = {sw, sw, sw, sw, 4, 4};
    int64_t top = 0;
    auto take = [&](int64_t bytes) {
        const int64_t o = top;
        top += align256(bytes > 0 ? bytes : 1);
        return o;
    };
    L.off_node_off = take(4 * (bs + 1));
    L.off_edge_off = take(4 * (bs + 1));
    L.off_totals = take(16);
    L.off_n_batch = take(8 * bs);
    L.off_e_batch = take(8 * bs);
    L.off_x = take(4 * L.nodes * L.f_in);
    L.off_xl = take(4 * L.edges);
    for (int k = 0; k < K_N; ++k) {
        L.rows[k] = (k >= K_WL && !L.dual) ? 0 : rows_of[k];
        L.off_rows[k] = take(8 * L.rows[k]);
        L.off_entries[k] = take(4 * stride_of[k] * L.nnz[k]);
    }
    L.bytes = top;
}
}  // namespace hgnn

extern "C" {

int hgnn_graph_edge_slots(int n, const float* A) {
    if (n < 0 || (n > 0 && !A)) return -1;
    return nnz_of(n, A);
}

int hgnn_graph_operators(int n, const float* A, int J, int dual, float* W, int m, float* WL, float* Pm, float* Pd) {
    if (n <= 0 || !A || !W || J < 1 || J > 5) return HGNN_ERR_ARG;
    const int jt = J + 2;
    const Sp a = adjacency(n, A);
    const Ops w = slices(a, jt);
    memset(W, 0, sizeof(float) * (size_t)n * n * jt);
    for (int r = 0; r < n; ++r)
        for (size_t e = 0; e < w.cols[r].size(); ++e)
            for (int j = 0; j < jt; ++j) W[((size_t)r * n + w.cols[r][e]) * jt + j] = w.vals[r][e * jt + j];
    if (!dual) return HGNN_OK;
    if (m != nnz_of(n, A) || (m > 0 && (!WL || !Pm || !Pd))) return HGNN_ERR_ARG;
    if (m == 0) return HGNN_OK;
    std::vector<Edge> edges;
    std::vector<float> pm, pd;
    if (!edge_slots(n, A, m, edges, &pm, &pd)) return HGNN_ERR_INDEX;
    memcpy(Pm, pm.data(), sizeof(float) * (size_t)n * m);
    memcpy(Pd, pd.data(), sizeof(float) * (size_t)n * m);
    const Ops wl = slices(line_graph(edges), jt);
    memset(WL, 0, sizeof(float) * (size_t)m * m * jt);
    for (int r = 0; r < m; ++r)
        for (size_t e = 0; e < wl.cols[r].size(); ++e)
            for (int j = 0; j < jt; ++j) WL[((size_t)r * m + wl.cols[r][e]) * jt + j] = wl.vals[r][e * jt + j];
    return HGNN_OK;
}

// Computes the layout; with `image`, writes it after checking it against `expect`
// (the layout the caller sized the image with).
static int csr_batch(int bs, const int* n_nodes, const float* const* A, const float* const* X, int f_in, int J,
                     int dual, const hgnn_csr_layout* expect, hgnn_csr_layout* lay, void* image) {
    if (bs <= 0 || !n_nodes || !A || !lay || f_in <= 0 || J < 1 || J > 5) return HGNN_ERR_ARG;
    const int jt = J + 2;
    const int sw = jt <= 3 ? 4 : 8;
    std::vector<GraphBuild> gs(bs);
    hgnn_csr_layout L;
    memset(&L, 0, sizeof(L));
    L.bs = bs;
    L.f_in = f_in;
    L.j_tot = jt;
    L.dual = dual ? 1 : 0;
    L.stride_w = sw;
    for (int b = 0; b < bs; ++b) {
        if (n_nodes[b] <= 0 || !A[b]) return HGNN_ERR_ARG;
        const int st = build_graph(n_nodes[b], A[b], jt, dual != 0, gs[b]);
        if (st) return st;
        L.nmax = std::max(L.nmax, gs[b].n);
        L.emax = std::max(L.emax, gs[b].m);
        L.nodes += gs[b].n;
        L.edges += gs[b].m;
        auto add = [&](int k, const Ops& o) {
            for (auto& c : o.cols) L.nnz[k] += (int64_t)c.size();
        };
        add(K_W, gs[b].W);
        add(K_WT, gs[b].WT);
        if (dual) {
            add(K_WL, gs[b].WL);
            add(K_WLT, gs[b].WLT);
            for (auto& r : gs[b].pn) L.nnz[K_PN] += (int64_t)r.size();
            for (auto& r : gs[b].pe) L.nnz[K_PE] += (int64_t)r.size();
        }
    }
    const int stride_of[K_N] = {sw, sw, sw, sw, 4, 4};
    hgnn::csr_layout_offsets(L);
    *lay = L;
    if (!image) return HGNN_OK;
    if (!expect || memcmp(expect, &L, sizeof(L)) != 0) return HGNN_ERR_ARG;

    char* img = static_cast<char*>(image);
    memset(img, 0, (size_t)L.bytes);
    int32_t* node_off = reinterpret_cast<int32_t*>(img + L.off_node_off);
    int32_t* edge_off = reinterpret_cast<int32_t*>(img + L.off_edge_off);
    int32_t* totals = reinterpret_cast<int32_t*>(img + L.off_totals);
    int64_t* nb = reinterpret_cast<int64_t*>(img + L.off_n_batch);
    int64_t* eb = reinterpret_cast<int64_t*>(img + L.off_e_batch);
    float* xp = reinterpret_cast<float*>(img + L.off_x);
    float* xl = reinterpret_cast<float*>(img + L.off_xl);
    Row* rows[K_N];
    float* ent[K_N];
    for (int k = 0; k < K_N; ++k) {
        rows[k] = reinterpret_cast<Row*>(img + L.off_rows[k]);
        ent[k] = reinterpret_cast<float*>(img + L.off_entries[k]);
    }
    int64_t fill[K_N] = {0, 0, 0, 0, 0, 0};
    auto put_ops = [&](int k, const Ops& o, int row0, int col0) {
        for (int r = 0; r < o.n; ++r) {
            rows[k][row0 + r] = Row{(int32_t)fill[k], (int32_t)o.cols[r].size()};
            for (size_t e = 0; e < o.cols[r].size(); ++e) {
                float* q = ent[k] + fill[k] * stride_of[k];
                const int32_t col = col0 + o.cols[r][e];
                memcpy(q, &col, 4);
                for (int j = 0; j < o.jt; ++j) q[1 + j] = o.vals[r][e * o.jt + j];
                ++fill[k];
            }
        }
    };
    auto put_inc = [&](int k, const std::vector<std::vector<std::pair<int, std::pair<float, float>>>>& rs, int row0,
                       int col0) {
        for (size_t r = 0; r < rs.size(); ++r) {
            rows[k][row0 + r] = Row{(int32_t)fill[k], (int32_t)rs[r].size()};
            for (auto& [c, v] : rs[r]) {
                float* q = ent[k] + fill[k] * 4;
                const int32_t col = col0 + c;
                memcpy(q, &col, 4);
                q[1] = v.first;
                q[2] = v.second;
                ++fill[k];
            }
        }
    };
    int n0 = 0, e0 = 0;
    for (int b = 0; b < bs; ++b) {
        const GraphBuild& g = gs[b];
        node_off[b] = n0;
        edge_off[b] = e0;
        nb[b] = g.n;
        eb[b] = g.m;
        if (X && X[b]) memcpy(xp + (size_t)n0 * f_in, X[b], sizeof(float) * (size_t)g.n * f_in);
        put_ops(K_W, g.W, n0, n0);
        put_ops(K_WT, g.WT, n0, n0);
        if (dual) {
            for (int r = 0; r < g.m; ++r) xl[e0 + r] = g.xl[r];
            put_ops(K_WL, g.WL, e0, e0);
            put_ops(K_WLT, g.WLT, e0, e0);
            put_inc(K_PN, g.pn, n0, e0);
            put_inc(K_PE, g.pe, e0, n0);
        }
        n0 += g.n;
        e0 += g.m;
    }
    node_off[bs] = n0;
    edge_off[bs] = e0;
    totals[0] = n0;
    totals[1] = e0;
    return HGNN_OK;
}

int hgnn_csr_batch_plan(int bs, const int* n_nodes, const float* const* A, int f_in, int J, int dual,
                        hgnn_csr_layout* layout) {
    return csr_batch(bs, n_nodes, A, nullptr, f_in, J, dual, nullptr, layout, nullptr);
}

int hgnn_csr_batch_build(int bs, const int* n_nodes, const float* const* A, const float* const* X, int f_in, int J,
                         int dual, const hgnn_csr_layout* layout, void* image) {
    if (!layout || !image) return HGNN_ERR_ARG;
    hgnn_csr_layout L;
    return csr_batch(bs, n_nodes, A, X, f_in, J, dual, layout, &L, image);
}

int hgnn_csr_layout_from_counts(int bs, const int32_t* counts, int f_in, int J, int dual, hgnn_csr_layout* layout) {
    if (bs <= 0 || !counts || !layout || f_in <= 0 || J < 1 || J > 5) return HGNN_ERR_ARG;
    const int jt = J + 2;
    hgnn_csr_layout L;
    memset(&L, 0, sizeof(L));
    L.bs = bs;
    L.f_in = f_in;
    L.j_tot = jt;
    L.dual = dual ? 1 : 0;
    L.stride_w = jt <= 3 ? 4 : 8;
    int flags = 0;
    for (int b = 0; b < bs; ++b) flags |= counts[(size_t)b * HGNN_PACK_COUNT_WORDS + 8];
    if (flags & HGNN_PACK_FLAG_INDEX) return HGNN_ERR_INDEX;
    if (flags & (HGNN_PACK_FLAG_BOUNDS | HGNN_PACK_FLAG_COO)) return HGNN_ERR_UNSUPPORTED;
    for (int b = 0; b < bs; ++b) {
        const int32_t* c = counts + (size_t)b * HGNN_PACK_COUNT_WORDS;
        if (c[0] <= 0 || c[1] < 0) return HGNN_ERR_ARG;
        L.nmax = std::max(L.nmax, c[0]);
        L.emax = std::max(L.emax, c[1]);
        L.nodes += c[0];
        L.edges += c[1];
        for (int k = 0; k < K_N; ++k) {
            if (c[2 + k] < 0) return HGNN_ERR_ARG;
            L.nnz[k] += c[2 + k];
        }
    }
    hgnn::csr_layout_offsets(L);
    *layout = L;
    return HGNN_OK;
}

}  // extern "C"
