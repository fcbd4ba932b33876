/* TEST INFRASTRUCTURE -- CPU restatement of umap-learn 0.5.x `optimize_layout_euclidean` (umap/layouts.py), the SGD
 * that `simplicial_set_embedding` runs for `sc.tl.umap` (call site: /root/reference/src/scanpy/tools/_umap.py:196-216;
 * umap-learn itself is NOT installed in the container: pyproject.toml pins `umap-learn>=0.5.12`).
 *
 * PARITY UNPINNED: the reference ships no golden embedding and the algorithm is stochastic; this file is the
 * published algorithm (McInnes et al. 2018, section 3.2 + the package's layouts.py as of 0.5) restated from memory:
 *   per epoch n, for every graph sample i = (j, k) with epoch_of_next_sample[i] <= n:
 *     attractive step on y_j (and y_k: move_other) with coefficient -2ab d^(2(b-1)) / (a d^(2b) + 1), clipped to +-4;
 *     int((n - epoch_of_next_negative_sample[i]) / epochs_per_negative_sample[i]) negative samples k' drawn with the
 *     per-vertex tau88 generator, repulsive coefficient 2 gamma b / ((0.001 + d^2)(a d^(2b) + 1));
 *   alpha = initial_alpha * (1 - n / n_epochs) after each epoch.
 * Three entry points (oracle_umap_synchronous_f64, at the end: the synchronous scheme with its forces in double):
 *   oracle_umap_sequential   -- the reference's sequential (Gauss-Seidel) sweep, `parallel=False`
 *   oracle_umap_synchronous  -- the SAME forces evaluated on a snapshot of the embedding per epoch (Jacobi), negatives
 *                               drawn from a counter-based hash: the scheme of scanpy_amd/csrc/umap.hip, restated on
 *                               the CPU so that the kernel can be checked element for element
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static inline float clip4(float v) { return v > 4.0f ? 4.0f : (v < -4.0f ? -4.0f : v); }

/* umap.utils.tau_rand_int: three-component Tausworthe generator on int64 state words (values kept to 32 bits) */
static inline int32_t tau_rand_int(int64_t* s) {
  s[0] = (((s[0] & 4294967294LL) << 12) & 0xffffffffLL) ^ ((((s[0] << 13) & 0xffffffffLL) ^ s[0]) >> 19);
  s[1] = (((s[1] & 4294967288LL) << 4) & 0xffffffffLL) ^ ((((s[1] << 2) & 0xffffffffLL) ^ s[1]) >> 25);
  s[2] = (((s[2] & 4294967280LL) << 17) & 0xffffffffLL) ^ ((((s[2] << 3) & 0xffffffffLL) ^ s[2]) >> 11);
  return (int32_t)(s[0] ^ s[1] ^ s[2]);
}

int oracle_umap_sequential(int64_t n_vertices, int dim, int64_t n_samples, const int32_t* head, const int32_t* tail,
                           const float* epochs_per_sample, int n_epochs, double a, double b, double gamma,
                           double initial_alpha, double negative_sample_rate, const int64_t* rng_state /*[3]*/,
                           float* y /* [n_vertices][dim], in/out */) {
  float* eps_neg = malloc(sizeof(float) * n_samples);
  float* next_neg = malloc(sizeof(float) * n_samples);
  float* next = malloc(sizeof(float) * n_samples);
  int64_t* rs = malloc(sizeof(int64_t) * 3 * n_vertices);
  if (!eps_neg || !next_neg || !next || !rs) return -1;
  for (int64_t i = 0; i < n_samples; ++i) {
    eps_neg[i] = epochs_per_sample[i] / (float)negative_sample_rate;
    next_neg[i] = eps_neg[i];
    next[i] = epochs_per_sample[i];
  }
  /* layouts.py: rng_state_per_sample = full((n_vertices, 3), rng_state) + head_embedding[:, 0].astype(float64).view(int64)... */
  for (int64_t v = 0; v < n_vertices; ++v) {
    double y0 = (double)y[v * dim];
    int64_t bits;
    memcpy(&bits, &y0, sizeof(bits));
    for (int t = 0; t < 3; ++t) rs[3 * v + t] = rng_state[t] + bits;
  }
  float alpha = (float)initial_alpha;
  for (int n = 0; n < n_epochs; ++n) {
    for (int64_t i = 0; i < n_samples; ++i) {
      if (next[i] > (float)n) continue;
      const int32_t j = head[i], k = tail[i];
      float* cur = y + (int64_t)j * dim;
      float* oth = y + (int64_t)k * dim;
      float d2 = 0.f;
      for (int t = 0; t < dim; ++t) d2 += (cur[t] - oth[t]) * (cur[t] - oth[t]);
      float coeff = 0.f;
      if (d2 > 0.f) {
        coeff = (float)(-2.0 * a * b * pow(d2, b - 1.0));
        coeff /= (float)(a * pow(d2, b) + 1.0);
      }
      for (int t = 0; t < dim; ++t) {
        const float g = clip4(coeff * (cur[t] - oth[t]));
        cur[t] += g * alpha;
        oth[t] += -g * alpha;
      }
      next[i] += epochs_per_sample[i];
      const int n_neg = (int)(((float)n - next_neg[i]) / eps_neg[i]);
      for (int p = 0; p < n_neg; ++p) {
        int64_t kk = (int64_t)tau_rand_int(rs + 3 * j) % n_vertices;
        if (kk < 0) kk += n_vertices; /* numba's % on a negative int32 follows Python: non-negative */
        float* o2 = y + kk * dim;
        float e2 = 0.f;
        for (int t = 0; t < dim; ++t) e2 += (cur[t] - o2[t]) * (cur[t] - o2[t]);
        float c2;
        if (e2 > 0.f) {
          c2 = (float)(2.0 * gamma * b);
          c2 /= (float)((0.001 + e2) * (a * pow(e2, b) + 1.0));
        } else if (j == kk) {
          continue;
        } else {
          c2 = 0.f;
        }
        for (int t = 0; t < dim; ++t) {
          const float g = c2 > 0.f ? clip4(c2 * (cur[t] - o2[t])) : 0.f;
          cur[t] += g * alpha;
        }
      }
      next_neg[i] += (float)n_neg * eps_neg[i];
    }
    alpha = (float)(initial_alpha * (1.0 - (double)n / (double)n_epochs));
  }
  free(eps_neg);
  free(next_neg);
  free(next);
  free(rs);
  return 0;
}

/* counter-based draw of the p-th negative sample of graph sample i at epoch n (same function as csrc/umap.hip) */
static inline uint32_t hash32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
static inline int64_t neg_vertex(uint64_t seed, int epoch, int64_t sample, int p, int64_t n_vertices) {
  uint32_t h = hash32((uint32_t)seed ^ hash32((uint32_t)(seed >> 32) + 0x9E3779B9U * (uint32_t)epoch));
  h = hash32(h ^ (uint32_t)sample);
  h = hash32(h + 0x85EBCA6BU * (uint32_t)(sample >> 32) + 0xC2B2AE35U * (uint32_t)p);
  return (int64_t)(((uint64_t)h * (uint64_t)n_vertices) >> 32);
}

/* Jacobi variant on the CSR of the symmetric graph: vertex v reads the epoch's snapshot y_in and writes y_out.
 * Row v holds the samples (v, u) with head v; the mirrored sample (u, v) has the same weight, hence the same firing
 * schedule, and its move_other step pulls v by the same clipped amount: the attractive step counts twice. */
int oracle_umap_synchronous(int64_t n_vertices, int dim, const int64_t* indptr, const int32_t* indices,
                            const float* epochs_per_sample, int n_epochs, double a, double b, double gamma,
                            double initial_alpha, double negative_sample_rate, uint64_t seed, float* y /* in/out */) {
  const int64_t n_samples = indptr[n_vertices];
  float* next = malloc(sizeof(float) * n_samples);
  float* next_neg = malloc(sizeof(float) * n_samples);
  float* y2 = malloc(sizeof(float) * n_vertices * dim);
  if (!next || !next_neg || !y2) return -1;
  for (int64_t i = 0; i < n_samples; ++i) {
    next[i] = epochs_per_sample[i];
    next_neg[i] = epochs_per_sample[i] / (float)negative_sample_rate;
  }
  float* yin = y;
  float* yout = y2;
  const float fa = (float)a, fb = (float)b, fg = (float)gamma;
  for (int n = 0; n < n_epochs; ++n) {
    /* the reference lowers alpha AFTER epoch n to initial_alpha (1 - n / n_epochs): epoch n >= 1 runs with the value
     * set after epoch n - 1 */
    const float alpha_n = (float)(initial_alpha * (1.0 - (double)(n > 0 ? n - 1 : 0) / (double)n_epochs));
    for (int64_t v = 0; v < n_vertices; ++v) {
      float delta[8] = {0};
      const float* cur = yin + v * dim;
      for (int64_t i = indptr[v]; i < indptr[v + 1]; ++i) {
        const float eps = epochs_per_sample[i];
        if (!(eps > 0.f) || next[i] > (float)n) continue;
        const float* oth = yin + (int64_t)indices[i] * dim;
        float d2 = 0.f;
        for (int t = 0; t < dim; ++t) d2 += (cur[t] - oth[t]) * (cur[t] - oth[t]);
        float coeff = 0.f;
        if (d2 > 0.f) coeff = (-2.0f * fa * fb * powf(d2, fb - 1.0f)) / (fa * powf(d2, fb) + 1.0f);
        for (int t = 0; t < dim; ++t) delta[t] += 2.0f * clip4(coeff * (cur[t] - oth[t]));
        next[i] += eps;
        const float eps_neg = eps / (float)negative_sample_rate;
        const int n_neg = (int)(((float)n - next_neg[i]) / eps_neg);
        for (int p = 0; p < n_neg; ++p) {
          const int64_t kk = neg_vertex(seed, n, i, p, n_vertices);
          if (kk == v) continue;
          const float* o2 = yin + kk * dim;
          float e2 = 0.f;
          for (int t = 0; t < dim; ++t) e2 += (cur[t] - o2[t]) * (cur[t] - o2[t]);
          if (e2 > 0.f) {
            const float c2 = (2.0f * fg * fb) / ((0.001f + e2) * (fa * powf(e2, fb) + 1.0f));
            for (int t = 0; t < dim; ++t) delta[t] += clip4(c2 * (cur[t] - o2[t]));
          }
        }
        next_neg[i] += (float)n_neg * eps_neg;
      }
      for (int t = 0; t < dim; ++t) yout[v * dim + t] = cur[t] + alpha_n * delta[t];
    }
    float* tmp = yin;
    yin = yout;
    yout = tmp;
  }
  if (yin != y) memcpy(y, yin, sizeof(float) * n_vertices * dim);
  free(next);
  free(next_neg);
  free(y2);
  return 0;
}

/* The same scheme with the FORCES in double: the schedule arithmetic (next, next_neg, eps_neg, n_neg) stays in float32,
 * operation for operation as above and as in csrc/umap.hip -- it does not depend on y, so which sample fires when, and how
 * many negatives it draws, is decided identically; the hash is the same.  Differences, pow, coefficients, clipping and sums
 * are double, and the embedding is held in double between the epochs (y is read once, rounded to float32 never; y64_out
 * takes the result).  sabs_out[v * dim + t] = the sum of |term| that went into coordinate t of vertex v in the LAST epoch
 * (attractive terms counted with their factor 2): alpha * 2^-23 * sabs is the unit in which the tests bound a float32
 * evaluation of that epoch. */
int oracle_umap_synchronous_f64(int64_t n_vertices, int dim, const int64_t* indptr, const int32_t* indices,
                                const float* epochs_per_sample, int n_epochs, double a, double b, double gamma,
                                double initial_alpha, double negative_sample_rate, uint64_t seed, const float* y,
                                double* y64_out, double* sabs_out) {
  const int64_t n_samples = indptr[n_vertices];
  float* next = malloc(sizeof(float) * (n_samples + 1));
  float* next_neg = malloc(sizeof(float) * (n_samples + 1));
  double* y2 = malloc(sizeof(double) * n_vertices * dim);
  if (!next || !next_neg || !y2) return -1;
  for (int64_t i = 0; i < n_samples; ++i) {
    next[i] = epochs_per_sample[i];
    next_neg[i] = epochs_per_sample[i] / (float)negative_sample_rate;
  }
  for (int64_t i = 0; i < n_vertices * dim; ++i) {
    y64_out[i] = (double)y[i];
    sabs_out[i] = 0.0;
  }
  double* yin = y64_out;
  double* yout = y2;
  /* the kernel receives a, b, gamma and alpha as float32: the same values, widened */
  const double fa = (double)(float)a, fb = (double)(float)b, fg = (double)(float)gamma;
  for (int n = 0; n < n_epochs; ++n) {
    const double alpha_n = (double)(float)(initial_alpha * (1.0 - (double)(n > 0 ? n - 1 : 0) / (double)n_epochs));
    for (int64_t v = 0; v < n_vertices; ++v) {
      double delta[8] = {0}, sabs[8] = {0};
      const double* cur = yin + v * dim;
      for (int64_t i = indptr[v]; i < indptr[v + 1]; ++i) {
        const float eps = epochs_per_sample[i];
        if (!(eps > 0.f) || next[i] > (float)n) continue;
        const double* oth = yin + (int64_t)indices[i] * dim;
        double d2 = 0.0;
        for (int t = 0; t < dim; ++t) d2 += (cur[t] - oth[t]) * (cur[t] - oth[t]);
        double coeff = 0.0;
        if (d2 > 0.0) {
          const double pw = pow(d2, fb);
          coeff = (-2.0 * fa * fb * (pw / d2)) / (fa * pw + 1.0);
        }
        for (int t = 0; t < dim; ++t) {
          double g = coeff * (cur[t] - oth[t]);
          g = 2.0 * (g > 4.0 ? 4.0 : (g < -4.0 ? -4.0 : g));
          delta[t] += g;
          sabs[t] += fabs(g);
        }
        next[i] += eps;
        const float eps_neg = eps / (float)negative_sample_rate;
        const int n_neg = (int)(((float)n - next_neg[i]) / eps_neg);
        for (int p = 0; p < n_neg; ++p) {
          const int64_t kk = neg_vertex(seed, n, i, p, n_vertices);
          if (kk == v) continue;
          const double* o2 = yin + kk * dim;
          double e2 = 0.0;
          for (int t = 0; t < dim; ++t) e2 += (cur[t] - o2[t]) * (cur[t] - o2[t]);
          if (e2 > 0.0) {
            const double c2 = (2.0 * fg * fb) / (((double)0.001f + e2) * (fa * pow(e2, fb) + 1.0));
            for (int t = 0; t < dim; ++t) {
              double g = c2 * (cur[t] - o2[t]);
              g = g > 4.0 ? 4.0 : (g < -4.0 ? -4.0 : g);
              delta[t] += g;
              sabs[t] += fabs(g);
            }
          }
        }
        next_neg[i] += (float)n_neg * eps_neg;
      }
      for (int t = 0; t < dim; ++t) {
        yout[v * dim + t] = cur[t] + alpha_n * delta[t];
        if (n == n_epochs - 1) sabs_out[v * dim + t] = sabs[t];
      }
    }
    double* tmp = yin;
    yin = yout;
    yout = tmp;
  }
  if (yin != y64_out) memcpy(y64_out, yin, sizeof(double) * n_vertices * dim);
  free(next);
  free(next_neg);
  free(y2);
  return 0;
}
