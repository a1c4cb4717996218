// Next-row f6: the reference's face clustering, kept on the device.  The reference copies the FaceNet embeddings of a video to the
// host, takes np.dot(E, E.T) (preprocessing/cluster_faces.py:96, predict.py:162), walks all n^2 entries in a Python double loop that
// adds an edge to a networkx graph wherever similarities[i, j] > threshold, and lists the connected components
// (_generate_connected_components, preprocessing/utils.py:16-29).  Here:
//   mt_identity_adjacency      32 x 32 tiles of each video's Gram matrix on v_mfma_f32_32x32x2_f32, compared with the threshold in the
//                              accumulator registers and packed with wave ballots into a bit matrix; no [n, n] float matrix exists
//   mt_identity_adjacency_sim  the same bit matrix from a ready similarity matrix of one video (the function's own argument)
//   mt_identity_components     one block per video: minimum-label propagation + pointer jumping on labels held in LDS, then the
//                              0-based rank of every component that has an edge, in order of its smallest member
// The rule (include/mintime_hip.h has it in full): i -- j iff i != j and s_ij > threshold (strict; NaN is no edge); a face without
// an edge is labelled -1 (the reference never adds it to the graph); the other faces get the rank of their component among the
// video's components in the order nx.connected_components yields them for that graph: by the first row of the double loop that
// adds one of the component's edges.  From embeddings (s_ij == s_ji) that row is the component's smallest member; from an asymmetric
// similarity matrix it is the smallest member i with some sim[i][j] > threshold ("source" below).
// The labelling is the unique minimum-member one, so the result does not depend on the schedule; the only atomics are integer
// (LDS member counts, the sticky error flag).  Nothing in this file reads back to the host.
#include "common.hpp"
#include <stdint.h>

namespace {
using namespace mt;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int ID_MAX_FACES = 4096;                     // labels of one video in LDS: 16 KB
constexpr int ID_MAX_DIM = 2048;
constexpr int ID_TILE = 32;                            // one wavefront = one 32 x 32 tile of the Gram matrix
constexpr int ID_KC = 32;                              // embedding columns staged per step of the K loop
constexpr int ID_PITCH = ID_KC + 1;
enum { ID_ERR_TRUNCATED = 1, ID_ERR_NOT_CONVERGED = 2, ID_ERR_OFFSETS = 4 };

// the 32 rows x ID_KC columns of `e` starting at column k0, zero beyond `rows` / D: lane l takes column l & 31 of rows
// (l >> 5) + 2 u, so every half wavefront reads 128 contiguous bytes
__device__ __forceinline__ void id_load_chunk(float (&r)[16], const float* __restrict__ e, int rows, int D, int k0, int lane) {
  const int kk = k0 + (lane & 31);
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int row = (lane >> 5) + 2 * u;
    r[u] = (row < rows && kk < D) ? e[(size_t)row * D + kk] : 0.f;
  }
}
__device__ __forceinline__ void id_store_chunk(float* s, const float (&r)[16], int lane) {
#pragma unroll
  for (int u = 0; u < 16; ++u) s[((lane >> 5) + 2 * u) * ID_PITCH + (lane & 31)] = r[u];
}

// Block b is tile (ti, tj) of the video v with tile_prefix[v] <= b < tile_prefix[v + 1].  s_ij accumulates e_ik * e_jk in
// ascending k as one fma chain (the MFMA takes k = 2 s from the lower half of the wavefront, then k = 2 s + 1 from the upper);
// s_ji is the same products in the same order, so the two triangles agree to the bit and the adjacency is symmetric.
__global__ __launch_bounds__(64) void identity_gram_adjacency_kernel(const float* __restrict__ emb, const int* __restrict__ offsets,
                                                                     const int* __restrict__ tile_prefix, int V, int T, int D,
                                                                     int max_faces, int W, float thr, unsigned* __restrict__ adj,
                                                                     int* __restrict__ err_flag) {
  __shared__ float sa[ID_TILE * ID_PITCH], sb[ID_TILE * ID_PITCH];
  const int lane = threadIdx.x, b = blockIdx.x;
  int lo = 0, hi = V;                                    // the number of videos whose first tile is <= b
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tile_prefix[mid] <= b) lo = mid + 1; else hi = mid;
  }
  const int v = lo - 1;
  if (v < 0) return;
  const int off = offsets[v], n_full = offsets[v + 1] - off;
  if (off < 0 || n_full <= 0 || off > T - n_full) return;           // (mt_identity_components reports bad offsets)
  const int n = n_full < max_faces ? n_full : max_faces;            // a longer video is truncated: rows and bits stay inside [T][W]
  const int nt = (n + ID_TILE - 1) / ID_TILE, local = b - tile_prefix[v];
  if (local == 0 && lane == 0 && n_full > max_faces && err_flag) atomicOr(err_flag, ID_ERR_TRUNCATED);
  if (local < 0 || local >= nt * nt) return;                        // a prefix that disagrees with the offsets launches idle blocks
  const int ti = local / nt, tj = local - ti * nt;
  const int r0 = ti * ID_TILE, c0 = tj * ID_TILE;
  const int rows_a = n - r0 < ID_TILE ? n - r0 : ID_TILE, rows_b = n - c0 < ID_TILE ? n - c0 : ID_TILE;
  const float* ea = emb + (size_t)(off + r0) * D;
  const float* eb = emb + (size_t)(off + c0) * D;
  const bool diag = ti == tj;                            // uniform: the tile's two operands are the same rows
  const float* pb = diag ? sa : sb;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float ra[16], rb[16];
  id_load_chunk(ra, ea, rows_a, D, 0, lane);
  if (!diag) id_load_chunk(rb, eb, rows_b, D, 0, lane);
  for (int k0 = 0; k0 < D; k0 += ID_KC) {
    __syncthreads();                                     // the previous chunk has been read
    id_store_chunk(sa, ra, lane);
    if (!diag) id_store_chunk(sb, rb, lane);
    __syncthreads();
    if (k0 + ID_KC < D) {                                // the next chunk's loads fly under this chunk's MFMAs
      id_load_chunk(ra, ea, rows_a, D, k0 + ID_KC, lane);
      if (!diag) id_load_chunk(rb, eb, rows_b, D, k0 + ID_KC, lane);
    }
    const int left = D - k0, steps = left >= ID_KC ? ID_KC / 2 : (left + 1) / 2;      // an odd D: a zero in the last step
    const int o = (lane & 31) * ID_PITCH + (lane >> 5);
    for (int s = 0; s < steps; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[o + 2 * s], pb[o + 2 * s], acc, 0, 0, 0);
  }

  // accumulator register r of a lane in half hf holds row mfma_slot_row(r, hf), column lane & 31: one ballot = two row words
  const int col = lane & 31, hf = lane >> 5;
  unsigned word = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = mfma_slot_row(r, hf);
    const bool e = col < rows_b && row < rows_a && (r0 + row != c0 + col) && acc[r] > thr;      // NaN > thr is false
    const unsigned long long m = __ballot(e);
    if (lane == mfma_slot_row(r, 0)) word = (unsigned)m;
    if (lane == mfma_slot_row(r, 1)) word = (unsigned)(m >> 32);
  }
  if (lane < rows_a) {
    unsigned* p = adj + (size_t)(off + r0 + lane) * W;
    p[tj] = word;
    if (tj == nt - 1)
      for (int w = nt; w < W; ++w) p[w] = 0u;            // the words past the video's last tile: every row is fully written
  }
}

// one wavefront per row, 64 columns per ballot.  The reference visits (i, j) and (j, i) and the graph is undirected: either order
// above the threshold is an edge.  source[i] = row i itself holds an entry above the threshold: the rows at which the reference's
// loop adds edges, which decide the order of the components.
__global__ __launch_bounds__(256) void identity_sim_adjacency_kernel(const float* __restrict__ sim, int n, int W, float thr,
                                                                     unsigned* __restrict__ adj, int* __restrict__ source) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                                    // (no barrier below)
  bool any_forward = false;
  for (int c0 = 0; c0 < W * 32; c0 += 64) {
    const int j = c0 + lane;
    bool fwd = false, e = false;
    if (j < n && j != i) {
      fwd = sim[(size_t)i * n + j] > thr;
      e = fwd || sim[(size_t)j * n + i] > thr;
    }
    const unsigned long long m = __ballot(e);
    any_forward |= __ballot(fwd) != 0ull;
    const int w = (c0 >> 5) + lane;
    if (lane < 2 && w < W) adj[(size_t)i * W + w] = lane ? (unsigned)(m >> 32) : (unsigned)m;
  }
  if (lane == 0) source[i] = any_forward ? 1 : 0;
}

constexpr int CC_THREADS = 1024, CC_ROWS = ID_MAX_FACES / CC_THREADS;

// Thread t owns faces t, t + 1024, ...  Every label is always the index of a member of the face's own component, and labels only
// fall, so the fixed point is label = smallest member.  Reads and writes of a step are separated by barriers.
__global__ __launch_bounds__(CC_THREADS) void identity_components_kernel(const unsigned* __restrict__ adj, const int* __restrict__ offsets,
                                                                         const int* __restrict__ source, int T, int max_faces, int W,
                                                                         int* __restrict__ labels, int* __restrict__ n_identities,
                                                                         int* __restrict__ sizes, int* __restrict__ err_flag) {
  __shared__ int lab[ID_MAX_FACES];
  __shared__ int key[ID_MAX_FACES];
  __shared__ int cnt[ID_MAX_FACES];
  __shared__ unsigned long long keybits[ID_MAX_FACES / 64];
  __shared__ int wordpre[ID_MAX_FACES / 64 + 1];
  __shared__ int changed;
  const int v = blockIdx.x, tid = threadIdx.x;
  const int off = offsets[v], n_full = offsets[v + 1] - off;
  if (off < 0 || n_full < 0 || off > T - n_full) {       // uniform: the whole block leaves
    if (tid == 0) {
      n_identities[v] = 0;
      if (err_flag) atomicOr(err_flag, ID_ERR_OFFSETS);
    }
    return;
  }
  const int n = n_full < max_faces ? n_full : max_faces;
  if (tid == 0 && n_full > max_faces && err_flag) atomicOr(err_flag, ID_ERR_TRUNCATED);
  const unsigned* A = adj + (size_t)off * W;
  const int nw = (n + 31) >> 5;

  bool has[CC_ROWS];
#pragma unroll
  for (int q = 0; q < CC_ROWS; ++q) {
    const int i = tid + q * CC_THREADS;
    has[q] = false;
    lab[i] = i;
    key[i] = ID_MAX_FACES;
    cnt[i] = 0;
  }
  if (tid < ID_MAX_FACES / 64) keybits[tid] = 0ull;
  __syncthreads();

  // n - 1 rounds of minimum propagation alone reach the fixed point and one more sees no change: the trip count is bounded
  bool converged = false;
  for (int round = 0; round <= n; ++round) {
    if (tid == 0) changed = 0;
    __syncthreads();
    int m[CC_ROWS];
#pragma unroll
    for (int q = 0; q < CC_ROWS; ++q) {
      const int i = tid + q * CC_THREADS;
      m[q] = lab[i];
      if (i < n) {
        const unsigned* row = A + (size_t)i * W;
        for (int w = 0; w < nw; ++w) {
          unsigned bits = row[w];
          if (bits) has[q] = true;
          // four neighbours per trip, so that four LDS reads are in flight; a spent mask repeats the first one.  Any bit of a
          // word below nw names a face below 4096, and lab[j] = j >= n for j >= n never wins the minimum: no bound check needed.
          const int* lw = lab + w * 32;
          while (bits) {
            const int j0 = __ffs(bits) - 1;
            bits &= bits - 1;
            const int j1 = bits ? __ffs(bits) - 1 : j0;
            bits &= bits - 1;
            const int j2 = bits ? __ffs(bits) - 1 : j0;
            bits &= bits - 1;
            const int j3 = bits ? __ffs(bits) - 1 : j0;
            bits &= bits - 1;
            m[q] = min(min(m[q], min(lw[j0], lw[j1])), min(lw[j2], lw[j3]));
          }
        }
      }
    }
    __syncthreads();
    bool ch = false;
#pragma unroll
    for (int q = 0; q < CC_ROWS; ++q) {
      const int i = tid + q * CC_THREADS;
      if (m[q] < lab[i]) { lab[i] = m[q]; ch = true; }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CC_ROWS; ++q) m[q] = lab[lab[tid + q * CC_THREADS]];          // pointer jump
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CC_ROWS; ++q) {
      const int i = tid + q * CC_THREADS;
      if (m[q] < lab[i]) { lab[i] = m[q]; ch = true; }
    }
    if (ch) changed = 1;
    __syncthreads();
    const int c = changed;
    __syncthreads();                                     // read by everyone before the next round clears it
    if (!c) { converged = true; break; }
  }
  if (!converged && tid == 0 && err_flag) atomicOr(err_flag, ID_ERR_NOT_CONVERGED);

  // A component's key = its smallest source (with no `source`, every face that has an edge is one: the key is the root itself).  An
  // edge has a source at one of its ends, so every component with an edge has a key; keys are distinct faces.  One bit per key: a
  // component's rank = the number of keys below its own.
#pragma unroll
  for (int q = 0; q < CC_ROWS; ++q) {
    const int i = tid + q * CC_THREADS;
    if (i < n && has[q] && (!source || source[off + i] != 0)) atomicMin(&key[lab[i]], i);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < CC_ROWS; ++q) {
    const int i = tid + q * CC_THREADS;
    if (i < n && has[q] && lab[i] == i && key[i] < n) atomicOr(&keybits[key[i] >> 6], 1ull << (key[i] & 63));
  }
  __syncthreads();
  if (tid < 64) {
    const int c = __popcll(keybits[tid]);
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (tid >= o) incl += t;
    }
    wordpre[tid] = incl - c;
    if (tid == 63) wordpre[64] = incl;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < CC_ROWS; ++q) {
    const int i = tid + q * CC_THREADS;
    if (i < n) {
      int rank = -1;
      const int k = has[q] ? key[lab[i]] : ID_MAX_FACES;
      if (k < n) {
        rank = wordpre[k >> 6] + __popcll(keybits[k >> 6] & ((1ull << (k & 63)) - 1ull));
        atomicAdd(&cnt[rank], 1);
      }
      labels[off + i] = rank;
    }
  }
  for (int i = n + tid; i < n_full; i += CC_THREADS) labels[off + i] = -1;            // faces past max_faces
  __syncthreads();
  if (sizes)
    for (int i = tid; i < n_full; i += CC_THREADS) sizes[off + i] = i < n ? cnt[i] : 0;
  if (tid == 0) n_identities[v] = wordpre[64];
}

int id_check_limits(const char* what, int max_faces) {
  if (max_faces < 1) return fail(MT_ERR_ARG, "%s: max_faces = %d", what, max_faces);
  if (max_faces > ID_MAX_FACES)
    return fail(MT_ERR_UNSUPPORTED, "%s: %d faces in one video; the labels of a video live in LDS: at most %d", what, max_faces, ID_MAX_FACES);
  return 0;
}

}  // namespace

extern "C" int mt_identity_adjacency(const float* emb, const int* offsets, const int* tile_prefix, int V, int T, int D, int total_tiles,
                                     int max_faces, float threshold, uint32_t* adj, int* err_flag, void* stream) {
  if (V < 1 || T < 0 || total_tiles < 0) return fail(MT_ERR_ARG, "mt_identity_adjacency: V = %d, T = %d, total_tiles = %d", V, T, total_tiles);
  if (const int rc = id_check_limits("mt_identity_adjacency", max_faces)) return rc;
  if (D < 1 || D > ID_MAX_DIM) return fail(MT_ERR_UNSUPPORTED, "mt_identity_adjacency: D = %d outside 1..%d", D, ID_MAX_DIM);
  if (!offsets || !tile_prefix || (T > 0 && (!emb || !adj))) return fail(MT_ERR_ARG, "mt_identity_adjacency: null pointer");
  if (total_tiles == 0 || T == 0) return 0;              // only empty videos: no tile, no row
  const int W = (max_faces + 31) / 32;
  hipLaunchKernelGGL(identity_gram_adjacency_kernel, dim3(total_tiles), dim3(64), 0, (hipStream_t)stream, emb, offsets, tile_prefix, V, T,
                     D, max_faces, W, threshold, reinterpret_cast<unsigned*>(adj), err_flag);
  return check_launch("mt_identity_adjacency");
}

extern "C" int mt_identity_adjacency_sim(const float* sim, int n, float threshold, uint32_t* adj, int* source, void* stream) {
  if (n < 0) return fail(MT_ERR_ARG, "mt_identity_adjacency_sim: n = %d", n);
  if (n == 0) return 0;
  if (const int rc = id_check_limits("mt_identity_adjacency_sim", n)) return rc;
  if (!sim || !adj || !source) return fail(MT_ERR_ARG, "mt_identity_adjacency_sim: null pointer");
  hipLaunchKernelGGL(identity_sim_adjacency_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, sim, n, (n + 31) / 32, threshold,
                     reinterpret_cast<unsigned*>(adj), source);
  return check_launch("mt_identity_adjacency_sim");
}

extern "C" int mt_identity_components(const uint32_t* adj, const int* offsets, const int* source, int V, int T, int max_faces, int* labels,
                                      int* n_identities, int* sizes, int* err_flag, void* stream) {
  if (V < 1 || T < 0) return fail(MT_ERR_ARG, "mt_identity_components: V = %d, T = %d", V, T);
  if (const int rc = id_check_limits("mt_identity_components", max_faces)) return rc;
  if (!offsets || !n_identities || (T > 0 && (!adj || !labels))) return fail(MT_ERR_ARG, "mt_identity_components: null pointer");
  hipLaunchKernelGGL(identity_components_kernel, dim3(V), dim3(CC_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const unsigned*>(adj),
                     offsets, source, T, max_faces, (max_faces + 31) / 32, labels, n_identities, sizes, err_flag);
  return check_launch("mt_identity_components");
}
