// llm_trie.hip -- trie-constrained token select of the native LLaMA engine (classify="constrained"; include/cgpt.h:
// "Trie-constrained answer decoding").
//
// Reference call replaced: HF `generate(..., prefix_allowed_tokens_fn=...)` over a vocabulary of candidate answers -- at every step
// the arg-max runs over the tokens that continue some candidate, and a row ends when it has spelled one.  The law is stated once in
// llm_laws.py (`constrained_select_law`); the greedy loop around the select is llm.hip's llm_greedy_entry, unchanged.
//
// The candidates are a CSR trie of int32 tables: the edges of node n are child_begin[n] .. child_begin[n + 1], edge e carries token
// child_tok[e] and leads to node child_node[e]; leaf_class[n] is the class id of a leaf and -1 on an inner node.  The edges of one
// node ascend strictly by token id, so "the first maximum over the edges" is "the lowest token id among the maxima".
// cgpt_llm_trie_check validates the tables on the host; the kernel trusts tables that passed it.
#include <stddef.h>

#include <string>
#include <vector>

#include "../../include/cgpt.h"
#include "common_host.h"
#include "llm_select.h"

using namespace cgpt;

namespace {

// One workgroup of 256 threads per row, the shape of llm_select_kernel.  The row's node comes from a.node[row] (a.first != 0: the
// root, and the row is unfinished).  The threads stride over the node's edges, gather src[row, child_tok[e]] and keep the first
// maximum; wave butterfly, then the four wave results through LDS, ties by the smaller edge index as llm_select_kernel breaks them
// by the smaller column.  One thread then moves the row to the child: node, unfinished, tokens_out, next_tok, and the label when the
// child is a leaf.  A finished row writes the pad id and nothing else.  GUARD (early stop): a select other than the first that reads
// *live == 0 writes the pad id and returns, as the arg-max's dead select does.
// A node outside 0 .. nodes-1 (a caller's own buffer: cgpt_llm_trie_select_logits) reads as the root, and a row standing on a leaf
// is treated as finished: nothing outside the tables is ever read.  Plain vector stores, no atomics.
template <bool GUARD>
__global__ __launch_bounds__(256) void llm_trie_select_kernel(TrieArgs a) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int row = blockIdx.x;
    if constexpr (GUARD) {
        if (!a.first && *a.live == 0) {
            if (threadIdx.x == 0) {
                a.tokens_out[(int64_t)row * a.ld_tokens] = a.pad;
                a.next_tok[row] = a.pad;
            }
            return;
        }
    }
    int n = a.first ? 0 : a.node[row];
    if (n < 0 || n >= a.nodes) n = 0;
    const int e0 = a.child_begin[n], e1 = a.child_begin[n + 1];
    const int u = a.first ? 1 : a.unfinished[row];
    if (!u || e1 <= e0) {                                  // uniform over the workgroup: no barrier has been passed
        if (threadIdx.x == 0) {
            a.tokens_out[(int64_t)row * a.ld_tokens] = a.pad;
            a.next_tok[row] = a.pad;
        }
        return;
    }
    const float* s = a.src + (int64_t)row * a.lds;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {
        const float v = s[a.child_tok[e]];
        if (idx == 0x7fffffff || v > best) { best = v; idx = e; }              // ascending e: the first maximum stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(idx, o);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
        if (idx < e0 || idx >= e1) idx = e0;               // unreachable for finite logits (thread 0 always holds edge e0)
        const int child = a.child_node[idx];
        const long long tok = a.child_tok[idx];
        const int cls = a.leaf_class[child];
        a.node[row] = child;
        a.unfinished[row] = cls < 0 ? 1 : 0;
        a.tokens_out[(int64_t)row * a.ld_tokens] = tok;
        a.next_tok[row] = tok;
        if (cls >= 0) a.labels_out[row] = cls;
    }
}

// dst[r, 0 .. cols) = src[r, 0 .. cols): the first logits into row 0 of the step-logits table (the trie select writes no copy).
__global__ __launch_bounds__(256) void llm_copy_rows_kernel(const float* __restrict__ src, int64_t lds, float* __restrict__ dst, int64_t ldd,
                                                            int cols) {
    const float* s = src + (int64_t)blockIdx.x * lds;
    float* d = dst + (int64_t)blockIdx.x * ldd;
    for (int j = blockIdx.y * 256 + threadIdx.x; j < cols; j += 256 * gridDim.y) d[j] = s[j];
}

}  // namespace

namespace cgpt {

hipError_t launch_llm_trie_select(bool guard, const TrieArgs& a, int rows, hipStream_t st) {
    if (guard)
        hipLaunchKernelGGL(llm_trie_select_kernel<true>, dim3(rows), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(llm_trie_select_kernel<false>, dim3(rows), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_llm_copy_rows(const float* src, int64_t lds, float* dst, int64_t ldd, int cols, int rows, hipStream_t st) {
    hipLaunchKernelGGL(llm_copy_rows_kernel, dim3(rows, 8), dim3(256), 0, st, src, lds, dst, ldd, cols);
    return hipGetLastError();
}

}  // namespace cgpt

extern "C" {

cgpt_status cgpt_llm_trie_check(const int32_t* child_begin, const int32_t* child_tok, const int32_t* child_node, const int32_t* leaf_class,
                                int32_t nodes, int32_t edges, int32_t vocab, int32_t* depth_out) {
    const std::string who = "cgpt_llm_trie_check";
    auto bad = [&](const std::string& msg) { return cgpt_fail(CGPT_ERR_INVALID, who + ": " + msg); };
    auto nd = [](int64_t n) { return "node " + std::to_string(n); };
    if (!child_begin || !child_tok || !child_node || !leaf_class) return bad("null table");
    if (vocab < 1) return bad("vocab < 1");
    if (nodes < 3 || nodes > TRIE_MAX_NODES)
        return bad(std::to_string(nodes) + " nodes (3.." + std::to_string(TRIE_MAX_NODES) + ": a root and at least 2 candidates)");
    if (edges != nodes - 1)
        return bad(std::to_string(edges) + " edges for " + std::to_string(nodes) + " nodes (every node but the root has one parent)");
    if (child_begin[0] != 0) return bad("node 0: child_begin[0] is not 0");
    for (int n = 0; n < nodes; ++n)
        if (child_begin[n + 1] < child_begin[n] || child_begin[n + 1] > edges)
            return bad(nd(n) + ": child_begin is not monotone within 0..edges");
    if (child_begin[nodes] != edges) return bad(nd(nodes - 1) + ": child_begin[nodes] != edges");
    std::vector<int> depth(nodes, -1), parents(nodes, 0);
    depth[0] = 0;
    int deepest = 0, leaves = 0;
    for (int n = 0; n < nodes; ++n) {                      // a parent comes before its children, so depth[n] is known here
        const int e0 = child_begin[n], e1 = child_begin[n + 1];
        if (n > 0 && parents[n] == 0) return bad(nd(n) + " is unreachable (no edge leads to it)");
        if (e0 == e1) {
            if (leaf_class[n] < 0) return bad(nd(n) + " is a leaf without a class (leaf_class < 0)");
            if (n == 0) return bad("node 0: the root has no children");
            ++leaves;
        } else if (leaf_class[n] != -1)
            return bad(nd(n) + " has children and a class (a candidate is a prefix of another; leaf_class must be -1)");
        for (int e = e0; e < e1; ++e) {
            if (child_tok[e] < 0 || child_tok[e] >= vocab)
                return bad(nd(n) + ": token " + std::to_string(child_tok[e]) + " outside 0.." + std::to_string(vocab - 1));
            if (e > e0 && child_tok[e] <= child_tok[e - 1])
                return bad(nd(n) + ": edge tokens are not strictly ascending (" + std::to_string(child_tok[e - 1]) + " then " +
                           std::to_string(child_tok[e]) + ")");
            const int c = child_node[e];
            if (c <= n || c >= nodes) return bad(nd(n) + ": child index " + std::to_string(c) + " is not in " + std::to_string(n + 1) + ".." +
                                                 std::to_string(nodes - 1));
            if (++parents[c] > 1) return bad(nd(c) + " has two parents");
            if (c != e + 1) return bad(nd(n) + ": child " + std::to_string(c) + " of edge " + std::to_string(e) + " is not numbered breadth-first");
            depth[c] = depth[n] + 1;
            if (depth[c] > deepest) deepest = depth[c];
        }
    }
    if (leaves < 2) return bad("fewer than 2 candidates");
    if (deepest > TRIE_MAX_DEPTH) return bad("depth " + std::to_string(deepest) + " > " + std::to_string(TRIE_MAX_DEPTH));
    if (depth_out) *depth_out = deepest;
    return CGPT_OK;
}

cgpt_status cgpt_llm_trie_select_logits(const float* logits_dev, int64_t ld, int32_t B, int32_t V, const int32_t* child_begin_dev,
                                        const int32_t* child_tok_dev, const int32_t* child_node_dev, const int32_t* leaf_class_dev,
                                        int32_t nodes, int64_t pad_id, int32_t* node_dev, int32_t* unfinished_dev,
                                        int64_t* tokens_out_dev, int32_t* labels_out_dev, void* stream) {
    const std::string who = "cgpt_llm_trie_select_logits";
    if (!logits_dev || !child_begin_dev || !child_tok_dev || !child_node_dev || !leaf_class_dev || !node_dev || !unfinished_dev ||
        !tokens_out_dev || !labels_out_dev)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": null argument");
    if (B < 1 || V < 1 || ld < V || nodes < 1 || nodes > TRIE_MAX_NODES)
        return cgpt_fail(CGPT_ERR_INVALID, who + ": B >= 1, V >= 1, ld >= V, nodes in 1.." + std::to_string(TRIE_MAX_NODES));
    TrieArgs a{logits_dev, ld, child_begin_dev, child_tok_dev, child_node_dev, leaf_class_dev, nodes, (long long)pad_id, 0, node_dev,
               unfinished_dev, (long long*)tokens_out_dev, 1, (long long*)tokens_out_dev, labels_out_dev, nullptr};
    hipError_t e = launch_llm_trie_select(false, a, B, (hipStream_t)stream);
    if (e != hipSuccess) return cgpt_fail(CGPT_ERR_HIP, who + ": launch -> " + hipGetErrorString(e));
    return CGPT_OK;
}

}  // extern "C"
