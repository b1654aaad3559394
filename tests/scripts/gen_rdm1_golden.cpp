// Producer of the fixtures tests/golden/rdm1_ref_<name>.txt: what the REFERENCE's one_elec_op (FRIES/Hamiltonians/molecule.cpp:222-252) and
// DistVec::internal_dot give for two small vectors and a list of orbital pairs.  Not collected by pytest and not part of the oracle; run
// once where the reference checkout lies ($REF, as in oracle/Makefile), after `make -C oracle ref`:
//
//   g++ -std=c++17 -O3 -msse4.2 -mpopcnt -ffp-contract=off -DMPICH_SKIP_MPICXX -pthread -I$REF -I$MPI_INC -o gen_rdm1_golden \
//       tests/scripts/gen_rdm1_golden.cpp -Loracle/_ref -lfries_ref $MPI_LIB/libmpi.so -Wl,-rpath-link,$MPI_LIB \
//       -Wl,-rpath,$PWD/oracle/_ref -Wl,-rpath,/usr/lib/x86_64-linux-gnu:$MPI_LIB
//   ./gen_rdm1_golden input.txt tests/golden/rdm1_ref_<name>.txt
//
// input.txt (the fixture repeats it, so the test needs nothing else):
//   NORB <n_orb> NELEC <n_elec>
//   A <determinant as an unsigned 64-bit integer> <value as a C99 hex float>      (one line per stored element of `a`)
//   B <determinant> <value>                                                       (... of `b`)
//   PAIR <des> <cre>                                                              (one line per orbital pair)
// The program puts b into column 0 and a into column 1 of one three-column DistVec<double>, prints internal_dot(0, 1) = <a|b> as
//   OVLP <hex float> <17 digits>
// and for every pair applies one_elec_op(vec, n_orb, des, cre, 2) and prints internal_dot(1, 2) = <a| sum_sigma c+_cre c_des |b> as
//   REF <des> <cre> <hex float> <17 digits>
// which is gamma(a, b)[cre][des] of fries_rdm1.  rdm1_ref_ne.txt: the vectors of two Ne-shaped frisys_mol runs (fcidump.synthetic("Ne"),
// seeds 1 and 2, 25 iterations at vec_nonz = mat_nonz = 150, max_dets = 4000, target_norm = 100, HB_unnorm), their non-zero elements.
#include <FRIES/vec_utils.hpp>
#include <FRIES/Hamiltonians/molecule.hpp>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s input.txt output.txt\n", argv[0]); return 2; }
    MPI_Init(NULL, NULL);
    unsigned n_orb = 0, n_elec = 0;
    std::vector<uint64_t> det[2]; std::vector<double> val[2];
    std::vector<std::pair<unsigned, unsigned>> pairs;
    std::vector<std::string> echo;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        echo.push_back(line);
        std::istringstream ss(line);
        std::string tag, t1, t2, t3;
        ss >> tag;
        if (tag == "NORB") { ss >> n_orb >> t1 >> n_elec; }
        else if (tag == "A" || tag == "B") { ss >> t1 >> t2; const int k = tag == "B"; det[k].push_back(strtoull(t1.c_str(), nullptr, 10)); val[k].push_back(strtod(t2.c_str(), nullptr)); }
        else if (tag == "PAIR") { unsigned d, c; ss >> d >> c; pairs.push_back({d, c}); }
        else { fprintf(stderr, "unknown line: %s\n", line.c_str()); return 2; }
    }
    if (!n_orb || !n_elec || det[0].empty() || det[1].empty() || pairs.empty()) { fprintf(stderr, "incomplete input\n"); return 2; }
    std::mt19937 rg(12345);
    std::vector<uint32_t> pscr(2 * n_orb), vscr(2 * n_orb);
    for (auto &x : pscr) x = rg();
    for (auto &x : vscr) x = rg();
    const size_t cap = 4 * (det[0].size() + det[1].size()) + 64;       // a, b and the targets of one pair (every call re-uses column 2; targets stay stored)
    std::function<double(const uint8_t *)> no_diag = [](const uint8_t *) { return 0.0; };
    DistVec<double> vec(cap * (pairs.size() + 1), cap, (uint8_t)(2 * n_orb), n_elec, 1, no_diag, 3, pscr, vscr);
    for (int col = 0; col < 2; col++) {         // column 0 <- b, column 1 <- a
        const int k = col == 0 ? 1 : 0;
        vec.set_curr_vec_idx((uint8_t)col);
        for (size_t i = 0; i < det[k].size(); i++) { uint8_t d[8]; memcpy(d, &det[k][i], 8); if (!vec.add(d, val[k][i], 1)) { fprintf(stderr, "adder full\n"); return 2; } }
        vec.perform_add(0);
    }
    vec.set_curr_vec_idx(0);
    FILE *f = fopen(argv[2], "w");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fprintf(f, "# one_elec_op (molecule.cpp:222-252) + DistVec::internal_dot of the reference on the vectors below: REF des cre = <a| sum_sigma c+_cre c_des |b>\n");
    for (const std::string &l : echo) fprintf(f, "%s\n", l.c_str());
    const double ov = vec.internal_dot(0, 1);
    fprintf(f, "OVLP %a %.17g\n", ov, ov);
    for (auto &pr : pairs) {
        one_elec_op(vec, n_orb, (uint8_t)pr.first, (uint8_t)pr.second, 2);
        const double g = vec.internal_dot(1, 2);
        fprintf(f, "REF %u %u %a %.17g\n", pr.first, pr.second, g, g);
    }
    fclose(f);
    printf("%zu + %zu elements, %zu pairs, %zu stored at the end\n", det[0].size(), det[1].size(), pairs.size(), (size_t)vec.curr_size());
    MPI_Finalize();
    return 0;
}
