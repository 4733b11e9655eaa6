// The 5-point essential-matrix solver, the RANSAC sample hash and the Sampson test of ransac.hip (header-inline, fp64,
// __host__ __device__ so that a host build can check the arithmetic the kernels run).
//
// Solver (Nister's elimination, written out here from the constraints):
//   1. The 5 correspondences give the 5x9 system x1^T E x0 = 0; its null space (Householder QR of the 9x5 transpose) is
//      spanned by X, Y, Z, W, and E = x X + y Y + z Z + W.
//   2. det E = 0 and 2 E E^T E - tr(E E^T) E = 0 are 10 cubics in (x, y, z): a 10x20 coefficient matrix over the monomials
//      in the order of MONO3 below, built by multiplying the linear entries of E as polynomials.
//   3. Gauss-Jordan (partial pivoting) on the first 10 columns.  The rows of x^2 z, y^2 z, x y z minus z times the rows of
//      x^2, y^2, x y are free of every eliminated monomial: three equations x p1(z) + y p2(z) + p3(z) = 0 with p1, p2 of
//      degree 3 and p3 of degree 4.  The determinant of that 3x3 matrix of polynomials is a polynomial of degree 10 in z.
//   4. Its real roots: every real root of a polynomial lies in one of the intervals cut by the real roots of its
//      derivative, where it is monotone, so the roots are found degree by degree (1 -> 10), each by a bracketed Newton /
//      bisection step inside one monotone interval.
//   5. Per root, (x, y, 1) spans the null space of the 3x3 matrix (cross product of its best-conditioned pair of rows);
//      E is scaled to unit Frobenius norm.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace e2emv {
namespace fivept {

#define FP_HD __host__ __device__ __forceinline__

// Counter-based sample hash (documented in include/e2emv.h, restated by the tests): the index of draw `draw` of iteration
// `iter` is floor(h * M / 2^32) with h = mix(mix(mix(seed ^ 0x9E3779B9) ^ iter) ^ draw).  The problem's batch position is
// not an input.
FP_HD uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}
FP_HD uint32_t sample_index(uint32_t seed, uint32_t iter, uint32_t draw, uint32_t M) {
    const uint32_t h = mix32(mix32(mix32(seed ^ 0x9E3779B9U) ^ iter) ^ draw);
    return (uint32_t)(((uint64_t)h * (uint64_t)M) >> 32);
}
// 5 distinct indices of [0, M): draws 0, 1, 2, ... in turn, a draw equal to an earlier pick is discarded.  After
// MAX_DRAWS draws without 5 distinct picks the iteration has no sample (returns false).
constexpr int MAX_DRAWS = 64;
FP_HD bool draw_sample(uint32_t seed, uint32_t iter, uint32_t M, int* idx) {
    int n = 0;
    for (uint32_t d = 0; d < (uint32_t)MAX_DRAWS && n < 5; ++d) {
        const int v = (int)sample_index(seed, iter, d, M);
        bool dup = false;
        for (int k = 0; k < n; ++k) dup |= idx[k] == v;
        if (!dup) idx[n++] = v;
    }
    return n == 5;
}

// squared Sampson distance of one correspondence against the inlier threshold t2 (= thresh^2), OpenCV's
// (x1^T E x0)^2 / ((E x0)_0^2 + (E x0)_1^2 + (E^T x1)_0^2 + (E^T x1)_1^2) <= t2, written without the division; a zero
// denominator is an outlier (the quotient would be NaN or inf)
FP_HD bool sampson_inlier(const double* E, double x0, double y0, double x1, double y1, double t2) {
    const double a0 = E[0] * x0 + E[1] * y0 + E[2], a1 = E[3] * x0 + E[4] * y0 + E[5], a2 = E[6] * x0 + E[7] * y0 + E[8];
    const double b0 = E[0] * x1 + E[3] * y1 + E[6], b1 = E[1] * x1 + E[4] * y1 + E[7];
    const double num = x1 * a0 + y1 * a1 + a2;
    const double den = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1;
    return den > 0.0 && num * num <= t2 * den;
}

// monomials of degree <= 3 in (x, y, z): the 10 eliminated ones first, then x{z^2,z,1}, y{z^2,z,1}, {z^3,z^2,z,1}
struct Mono { int a, b, c; };
constexpr Mono MONO3[20] = {{3, 0, 0}, {0, 3, 0}, {2, 1, 0}, {1, 2, 0}, {2, 0, 1}, {2, 0, 0}, {0, 2, 1}, {0, 2, 0}, {1, 1, 1},
                            {1, 1, 0}, {1, 0, 2}, {1, 0, 1}, {1, 0, 0}, {0, 1, 2}, {0, 1, 1}, {0, 1, 0}, {0, 0, 3}, {0, 0, 2},
                            {0, 0, 1}, {0, 0, 0}};
// linear (x, y, z, 1) and quadratic monomials
constexpr Mono MONO1[4] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}};
constexpr Mono MONO2[10] = {{2, 0, 0}, {1, 1, 0}, {1, 0, 1}, {0, 2, 0}, {0, 1, 1}, {0, 0, 2}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}};
FP_HD constexpr int idx2(int a, int b, int c) {
    for (int i = 0; i < 10; ++i)
        if (MONO2[i].a == a && MONO2[i].b == b && MONO2[i].c == c) return i;
    return -1;
}
FP_HD constexpr int idx3(int a, int b, int c) {
    for (int i = 0; i < 20; ++i)
        if (MONO3[i].a == a && MONO3[i].b == b && MONO3[i].c == c) return i;
    return -1;
}

FP_HD void mul11(const double* p, const double* q, double* out) {  // linear x linear -> quadratic (accumulates)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            out[idx2(MONO1[i].a + MONO1[j].a, MONO1[i].b + MONO1[j].b, MONO1[i].c + MONO1[j].c)] += p[i] * q[j];
}
FP_HD void mul21(const double* p, const double* q, double s, double* out) {  // s * quadratic x linear -> cubic (accumulates)
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            out[idx3(MONO2[i].a + MONO1[j].a, MONO2[i].b + MONO1[j].b, MONO2[i].c + MONO1[j].c)] += s * p[i] * q[j];
}

// ---- univariate polynomials, coefficients in ascending powers ----
FP_HD double horner(const double* c, int d, double x) {
    double v = c[d];
    for (int i = d - 1; i >= 0; --i) v = v * x + c[i];
    return v;
}
FP_HD void pmul(const double* a, int da, const double* b, int db, double* out) {  // out has da+db+1 entries (overwritten)
    for (int i = 0; i <= da + db; ++i) out[i] = 0.0;
    for (int i = 0; i <= da; ++i)
        for (int j = 0; j <= db; ++j) out[i + j] += a[i] * b[j];
}

// the root of c (degree d) in [lo, hi], where c is monotone and c(lo), c(hi) differ in sign: Newton steps kept inside the
// bracket and at least halving the step of the one before, bisection otherwise
FP_HD double bracketed_root(const double* c, int d, double lo, double hi, double flo) {
    double x = 0.5 * (lo + hi), prev_step = hi - lo;
    for (int it = 0; it < 200; ++it) {
        double f = c[d], df = 0.0;
        for (int i = d - 1; i >= 0; --i) {
            df = df * x + f;
            f = f * x + c[i];
        }
        if (f == 0.0) return x;
        if ((f < 0.0) == (flo < 0.0)) lo = x; else hi = x;
        double xn = x - f / df;
        if (!(xn > lo && xn < hi) || !(fabs(xn - x) <= 0.5 * prev_step)) xn = 0.5 * (lo + hi);
        const double step = fabs(xn - x);
        prev_step = step;
        x = xn;
        if (step <= 1e-15 * fabs(x) || step == 0.0 || !(lo < hi)) break;
    }
    return x;
}

// real roots of c (degree <= 10, ascending), sorted ascending; returns their number
FP_HD int real_roots10(const double* c_in, double* roots) {
    double c[11];
    double big = 0.0;
    for (int i = 0; i <= 10; ++i) {
        c[i] = c_in[i];
        big = fmax(big, fabs(c[i]));
    }
    if (!(big > 0.0) || !(big < 1e300)) return 0;  // zero or non-finite polynomial
    int d = 10;
    while (d > 0 && fabs(c[d]) <= 1e-15 * big) --d;
    if (d == 0) return 0;
    for (int i = 0; i <= d; ++i) c[i] /= c[d];
    double bound = 0.0;  // Cauchy: every root has |z| <= 1 + max |c_i / c_d|
    for (int i = 0; i < d; ++i) bound = fmax(bound, fabs(c[i]));
    bound += 1.0;
    // derivatives: der[k] = c^(k) / k!-free scaling (any positive multiple has the same roots)
    double der[11][11];
    for (int i = 0; i <= d; ++i) der[0][i] = c[i];
    for (int k = 1; k < d; ++k)
        for (int i = 0; i <= d - k; ++i) der[k][i] = der[k - 1][i + 1] * (double)(i + 1);
    // roots of der[d-1] (linear), then der[d-2], ..., der[0]
    double r[10];
    int nr = 0;
    {
        const double* l = der[d - 1];
        const double z = -l[0] / l[1];
        if (z > -bound && z < bound) r[nr++] = z;
    }
    for (int k = d - 2; k >= 0; --k) {
        const double* p = der[k];
        const int dk = d - k;
        double nxt[10];
        int nn = 0;
        double lo = -bound, flo = horner(p, dk, lo);
        for (int s = 0; s <= nr; ++s) {
            const double hi = (s < nr) ? r[s] : bound;
            const double fhi = horner(p, dk, hi);
            if (flo == 0.0) {
                if (nn == 0 || nxt[nn - 1] != lo) nxt[nn++] = lo;
            } else if ((flo < 0.0) != (fhi < 0.0) && fhi != 0.0) {
                nxt[nn++] = bracketed_root(p, dk, lo, hi, flo);
            }
            lo = hi;
            flo = fhi;
        }
        if (flo == 0.0 && (nn == 0 || nxt[nn - 1] != lo)) nxt[nn++] = lo;
        nr = nn;
        for (int i = 0; i < nr; ++i) r[i] = nxt[i];
    }
    for (int i = 0; i < nr; ++i) roots[i] = r[i];
    return nr;
}

// Null space of the 5x9 system: 4 orthonormal vectors N[4][9] (Householder QR of A^T).
FP_HD void nullspace5x9(const double (&A)[5][9], double (&N)[4][9]) {
    double v[5][9], beta[5];
    double M[9][5];
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 5; ++j) M[i][j] = A[j][i];
    for (int j = 0; j < 5; ++j) {
        double nrm = 0.0;
        for (int i = j; i < 9; ++i) nrm += M[i][j] * M[i][j];
        nrm = sqrt(nrm);
        for (int i = 0; i < 9; ++i) v[j][i] = 0.0;
        beta[j] = 0.0;
        if (nrm == 0.0) continue;
        const double alpha = M[j][j] >= 0.0 ? -nrm : nrm;
        for (int i = j; i < 9; ++i) v[j][i] = M[i][j];
        v[j][j] -= alpha;
        double vv = 0.0;
        for (int i = j; i < 9; ++i) vv += v[j][i] * v[j][i];
        if (vv == 0.0) continue;
        beta[j] = 2.0 / vv;
        for (int k = j; k < 5; ++k) {
            double s = 0.0;
            for (int i = j; i < 9; ++i) s += v[j][i] * M[i][k];
            s *= beta[j];
            for (int i = j; i < 9; ++i) M[i][k] -= s * v[j][i];
        }
    }
    for (int k = 0; k < 4; ++k) {  // Q e_{5+k} = H0 H1 ... H4 e_{5+k}
        double y[9];
        for (int i = 0; i < 9; ++i) y[i] = (i == 5 + k) ? 1.0 : 0.0;
        for (int j = 4; j >= 0; --j) {
            double s = 0.0;
            for (int i = j; i < 9; ++i) s += v[j][i] * y[i];
            s *= beta[j];
            for (int i = j; i < 9; ++i) y[i] -= s * v[j][i];
        }
        for (int i = 0; i < 9; ++i) N[k][i] = y[i];
    }
}

// Polishes a root (x, y, z) of the 10 cubics C . m(x, y, z) = 0 (rows of the reduced 10x20 system): Gauss-Newton steps
// on the 10x3 Jacobian.  The degree-10 polynomial loses digits where its roots crowd; the cubics do not.
FP_HD void gauss_newton3(const double (&C)[10][20], double& x, double& y, double& z) {
    double bx = x, by = y, bz = z, br2 = 1e308;  // the best point so far: a step that does not lower the residual ends the polish
    for (int it = 0; it < 6; ++it) {
        double px[4] = {1.0, x, x * x, x * x * x}, py[4] = {1.0, y, y * y, y * y * y}, pz[4] = {1.0, z, z * z, z * z * z};
        double m[20], mx[20], my[20], mz[20];
#pragma unroll
        for (int k = 0; k < 20; ++k) {
            const int a = MONO3[k].a, b = MONO3[k].b, c = MONO3[k].c;
            m[k] = px[a] * py[b] * pz[c];
            mx[k] = a ? a * px[a - 1] * py[b] * pz[c] : 0.0;
            my[k] = b ? b * px[a] * py[b - 1] * pz[c] : 0.0;
            mz[k] = c ? c * px[a] * py[b] * pz[c - 1] : 0.0;
        }
        double JtJ[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, Jtr[3] = {0.0, 0.0, 0.0}, r2 = 0.0;
        for (int r = 0; r < 10; ++r) {
            double f = 0.0, j[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < 20; ++k) {
                f += C[r][k] * m[k];
                j[0] += C[r][k] * mx[k];
                j[1] += C[r][k] * my[k];
                j[2] += C[r][k] * mz[k];
            }
            r2 += f * f;
            for (int a = 0; a < 3; ++a) {
                Jtr[a] += j[a] * f;
                for (int b = 0; b < 3; ++b) JtJ[a][b] += j[a] * j[b];
            }
        }
        // Cramer's rule on the 3x3 normal equations; a singular or non-finite step leaves the root as it is
        const double d = JtJ[0][0] * (JtJ[1][1] * JtJ[2][2] - JtJ[1][2] * JtJ[2][1]) -
                         JtJ[0][1] * (JtJ[1][0] * JtJ[2][2] - JtJ[1][2] * JtJ[2][0]) +
                         JtJ[0][2] * (JtJ[1][0] * JtJ[2][1] - JtJ[1][1] * JtJ[2][0]);
        if (!(r2 < br2)) break;
        bx = x; by = y; bz = z; br2 = r2;
        if (!(fabs(d) > 1e-300) || !(r2 > 0.0)) break;
        double dl[3];
        for (int c = 0; c < 3; ++c) {
            double M[3][3];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) M[a][b] = (b == c) ? -Jtr[a] : JtJ[a][b];
            dl[c] = (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                     M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0])) / d;
        }
        if (!(fabs(dl[0]) + fabs(dl[1]) + fabs(dl[2]) < 1e300)) break;
        x += dl[0];
        y += dl[1];
        z += dl[2];
    }
    x = bx;
    y = by;
    z = bz;
}

// All real essential matrices (row-major, unit Frobenius norm) of 5 correspondences (x0[k], y0[k]) <-> (x1[k], y1[k]) in
// normalised coordinates.  Returns their number (0..10).
FP_HD int solve5(const double* x0, const double* y0, const double* x1, const double* y1, double (*Es)[9]) {
    double A[5][9];
    for (int k = 0; k < 5; ++k) {
        const double p[3] = {x0[k], y0[k], 1.0}, q[3] = {x1[k], y1[k], 1.0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) A[k][3 * i + j] = q[i] * p[j];
    }
    double N[4][9];
    nullspace5x9(A, N);
    // entries of E as linear polynomials in (x, y, z, 1)
    double e[9][4];
    for (int k = 0; k < 9; ++k) {
        e[k][0] = N[0][k];
        e[k][1] = N[1][k];
        e[k][2] = N[2][k];
        e[k][3] = N[3][k];
    }
    double C[10][20];
    for (int r = 0; r < 10; ++r)
        for (int m = 0; m < 20; ++m) C[r][m] = 0.0;
    // det E by the first row's cofactors
    {
        double q[10];
        const int cof[3][4] = {{4, 8, 5, 7}, {3, 8, 5, 6}, {3, 7, 4, 6}};  // minor of E0j: e[a]e[b] - e[c]e[d]
        const double sg[3] = {1.0, -1.0, 1.0};
        for (int j = 0; j < 3; ++j) {
            for (int i = 0; i < 10; ++i) q[i] = 0.0;
            mul11(e[cof[j][0]], e[cof[j][1]], q);
            double q2[10];
            for (int i = 0; i < 10; ++i) q2[i] = 0.0;
            mul11(e[cof[j][2]], e[cof[j][3]], q2);
            for (int i = 0; i < 10; ++i) q[i] -= q2[i];
            mul21(q, e[j], sg[j], C[0]);
        }
    }
    // E E^T (quadratic), its trace, and 2 E E^T E - tr(E E^T) E (9 cubics)
    double Q[3][3][10];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            for (int m = 0; m < 10; ++m) Q[i][j][m] = 0.0;
            if (j < i) continue;
            for (int k = 0; k < 3; ++k) mul11(e[3 * i + k], e[3 * j + k], Q[i][j]);
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < i; ++j)
            for (int m = 0; m < 10; ++m) Q[i][j][m] = Q[j][i][m];
    double tr[10];
    for (int m = 0; m < 10; ++m) tr[m] = Q[0][0][m] + Q[1][1][m] + Q[2][2][m];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double* row = C[1 + 3 * i + j];
            for (int k = 0; k < 3; ++k) mul21(Q[i][k], e[3 * k + j], 2.0, row);
            mul21(tr, e[3 * i + j], -1.0, row);
        }
    // Gauss-Jordan on the first 10 columns
    for (int col = 0; col < 10; ++col) {
        int piv = col;
        double best = fabs(C[col][col]);
        for (int r = col + 1; r < 10; ++r)
            if (fabs(C[r][col]) > best) {
                best = fabs(C[r][col]);
                piv = r;
            }
        if (!(best > 1e-300)) return 0;  // degenerate sample
        if (piv != col)
            for (int m = 0; m < 20; ++m) {
                const double t = C[col][m];
                C[col][m] = C[piv][m];
                C[piv][m] = t;
            }
        const double inv = 1.0 / C[col][col];
        for (int m = col; m < 20; ++m) C[col][m] *= inv;
        for (int r = 0; r < 10; ++r) {
            if (r == col) continue;
            const double f = C[r][col];
            if (f == 0.0) continue;
            for (int m = col; m < 20; ++m) C[r][m] -= f * C[col][m];
        }
    }
    // rows (x^2 z, x^2), (y^2 z, y^2), (x y z, x y): row_a - z row_b over x{z^2,z,1}, y{z^2,z,1}, {z^3,z^2,z,1}
    double px[3][4], py[3][4], p1[3][5];
    const int pa[3] = {4, 6, 8}, pb[3] = {5, 7, 9};
    for (int r = 0; r < 3; ++r) {
        const double* a = C[pa[r]];
        const double* b = C[pb[r]];
        px[r][0] = a[12]; px[r][1] = a[11] - b[12]; px[r][2] = a[10] - b[11]; px[r][3] = -b[10];
        py[r][0] = a[15]; py[r][1] = a[14] - b[15]; py[r][2] = a[13] - b[14]; py[r][3] = -b[13];
        p1[r][0] = a[19]; p1[r][1] = a[18] - b[19]; p1[r][2] = a[17] - b[18]; p1[r][3] = a[16] - b[17]; p1[r][4] = -b[16];
    }
    // det of [[px0 py0 p10], [px1 py1 p11], [px2 py2 p12]] (degree 10)
    double poly[11], t7a[8], t7b[8], t6a[7], t6b[7], t10[11];
    for (int i = 0; i < 11; ++i) poly[i] = 0.0;
    pmul(py[1], 3, p1[2], 4, t7a);
    pmul(p1[1], 4, py[2], 3, t7b);
    for (int i = 0; i < 8; ++i) t7a[i] -= t7b[i];
    pmul(px[0], 3, t7a, 7, t10);
    for (int i = 0; i < 11; ++i) poly[i] += t10[i];
    pmul(px[1], 3, p1[2], 4, t7a);
    pmul(p1[1], 4, px[2], 3, t7b);
    for (int i = 0; i < 8; ++i) t7a[i] -= t7b[i];
    pmul(py[0], 3, t7a, 7, t10);
    for (int i = 0; i < 11; ++i) poly[i] -= t10[i];
    pmul(px[1], 3, py[2], 3, t6a);
    pmul(py[1], 3, px[2], 3, t6b);
    for (int i = 0; i < 7; ++i) t6a[i] -= t6b[i];
    pmul(p1[0], 4, t6a, 6, t10);
    for (int i = 0; i < 11; ++i) poly[i] += t10[i];
    double zs[10];
    const int nz = real_roots10(poly, zs);
    int ns = 0;
    for (int s = 0; s < nz; ++s) {
        const double z = zs[s];
        double B[3][3];
        for (int r = 0; r < 3; ++r) {
            B[r][0] = horner(px[r], 3, z);
            B[r][1] = horner(py[r], 3, z);
            B[r][2] = horner(p1[r], 4, z);
        }
        double v[3] = {0.0, 0.0, 0.0}, vn = -1.0;
        const int pr[3][2] = {{0, 1}, {0, 2}, {1, 2}};
        for (int k = 0; k < 3; ++k) {
            const double* a = B[pr[k][0]];
            const double* b = B[pr[k][1]];
            const double c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2], c2 = a[0] * b[1] - a[1] * b[0];
            const double n = c0 * c0 + c1 * c1 + c2 * c2;
            if (n > vn) {
                vn = n;
                v[0] = c0; v[1] = c1; v[2] = c2;
            }
        }
        if (!(fabs(v[2]) > 1e-300)) continue;
        double x = v[0] / v[2], y = v[1] / v[2], zz = z;
        gauss_newton3(C, x, y, zz);
        double En[9], nrm = 0.0;
        for (int k = 0; k < 9; ++k) {
            En[k] = x * N[0][k] + y * N[1][k] + zz * N[2][k] + N[3][k];
            nrm += En[k] * En[k];
        }
        if (!(nrm > 0.0) || !(nrm < 1e300)) continue;
        nrm = 1.0 / sqrt(nrm);
        for (int k = 0; k < 9; ++k) Es[ns][k] = En[k] * nrm;
        ++ns;
    }
    return ns;
}

#undef FP_HD

}  // namespace fivept
}  // namespace e2emv
