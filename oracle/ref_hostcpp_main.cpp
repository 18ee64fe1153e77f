// Harness around the reference's host-side attention check functions (TEST INFRASTRUCTURE ONLY).
//
// oracle/ref_hostcpp.py cuts the two functions out of the reference tree at run time into
// ref_hostcpp_cut.inc next to a copy of this file (both under oracle/_ref/, never committed) and
// compiles the pair.  This file is the project's own text: argument parsing and raw fp32 file io.
//
//   ref_hostcpp M N D scale causal in.bin out.bin
//     in.bin   Q [M,D]  K [N,D]  V [N,D]  dO [M,D]                 raw fp32, row-major
//     out.bin  O [M,D]  LSE [M]  dQ [M,D]  dK [N,D]  dV [N,D]      raw fp32, row-major
//
// The backward is given the forward's own fp32 O (it takes D_row = rowsum(O * dO) from it).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ref_hostcpp_cut.inc"

static void read_all(FILE* f, std::vector<float>& x) {
    if (fread(x.data(), sizeof(float), x.size(), f) != x.size()) {
        fprintf(stderr, "ref_hostcpp: short read\n");
        exit(2);
    }
}

static void write_all(FILE* f, const std::vector<float>& x) {
    if (fwrite(x.data(), sizeof(float), x.size(), f) != x.size()) {
        fprintf(stderr, "ref_hostcpp: short write\n");
        exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc != 8) {
        fprintf(stderr, "usage: %s M N D scale causal in.bin out.bin\n", argv[0]);
        return 2;
    }
    const int M = atoi(argv[1]), N = atoi(argv[2]), D = atoi(argv[3]);
    const float scale = strtof(argv[4], nullptr);
    const bool causal = atoi(argv[5]) != 0;
    if (M <= 0 || N <= 0 || D <= 0) {
        fprintf(stderr, "ref_hostcpp: M, N, D must be positive\n");
        return 2;
    }
    const size_t md = (size_t)M * D, nd = (size_t)N * D;
    std::vector<float> q(md), k(nd), v(nd), d_o(md);
    FILE* fi = fopen(argv[6], "rb");
    if (!fi) { perror(argv[6]); return 2; }
    read_all(fi, q); read_all(fi, k); read_all(fi, v); read_all(fi, d_o);
    fclose(fi);

    std::vector<float> o(md), lse(M), dq(md), dk(nd), dv(nd);
    cpu_attention_forward(q, k, v, o, lse, M, N, D, scale, causal);
    cpu_attention_backward(q, k, v, o, d_o, dq, dk, dv, M, N, D, scale, causal);

    FILE* fo = fopen(argv[7], "wb");
    if (!fo) { perror(argv[7]); return 2; }
    write_all(fo, o); write_all(fo, lse); write_all(fo, dq); write_all(fo, dk); write_all(fo, dv);
    fclose(fo);
    return 0;
}
