// Drives Dune::HipCGSolver's block apply (several right-hand sides at once, ddm_cg_solve_multi) the way examples/poisson.cc:229-321
// builds the solver: SchwarzPreconditioner (ILU(0)) + POU GalerkinPreconditioner in a CombinedPreconditioner, NonOverlappingOperator,
// CG on the device.  Single rank (mock communication, see mock/).  The block solve is checked against one device solve per column.
//   usage: multi_rhs_adaptor <dir with rowptr.bin col.bin val.bin b.bin dirichlet.bin pou.bin> <m>
// prints "col <c> <iterations block> <iterations single> <max |x_block - x_single|> <max |x_single|>" per column, then "block_ok".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "adaptor_fixture.hh"   // first: the adaptor headers below expect the dune-istl ones before them

#include <dune/ddm/hip/solvers.hh>

int main(int argc, char** argv)
{
  if (argc < 3) return 2;
  const std::string dir = argv[1];
  const int m = std::atoi(argv[2]);
  try {
    const Problem p = read_problem(dir);
    const auto bb = slurp<double>(dir + "/b.bin");
    const std::size_t n = p.n;
    const auto ptree = two_level_ptree("standard", "ilu0", "additive", "umfpack");
    const TwoLevel t = build_two_level(p, ptree);
    Dune::HipCGSolver<Vec> solver(t.op, t.prec, 1e-10, 500);

    std::vector<Vec> B = seeded_columns(p, bb, m), X = zero_columns(n, m);
    std::vector<Vec> Bsave = B;
    std::vector<Dune::InverseOperatorResult> res;
    solver.apply(X, B, 1e-10, res);   // one upload, one block solve, one download
    bool ok = res.size() == (std::size_t)m;
    for (int c = 0; c < m; ++c) {
      Vec x1(n), b1 = Bsave[c];
      x1 = 0;
      Dune::InverseOperatorResult r1;
      solver.apply(x1, b1, 1e-10, r1);   // the single-vector device solve of the same column
      double diff = 0.0, mx = 0.0;
      for (std::size_t i = 0; i < n; ++i) {
        diff = std::max(diff, std::fabs(X[c][i] - x1[i]));
        mx = std::max(mx, std::fabs(x1[i]));
      }
      std::printf("col %d %d %d %.3e %.3e\n", c, res[c].iterations, r1.iterations, diff, mx);
      ok = ok && res[c].converged && r1.converged && res[c].iterations == r1.iterations && diff <= 1e-8 * mx;
    }
    int caught = 0;
    try {
      std::vector<Vec> x0, b0;
      solver.apply(x0, b0, 1e-10, res);
    } catch (Dune::InvalidStateException&) { ++caught; }
    std::printf("errors_caught %d\n", caught);
    if (ok && caught == 1) std::printf("block_ok\n");
    return ok && caught == 1 ? 0 : 1;
  } catch (Dune::Exception& e) {
    std::cerr << "Dune exception: " << e.what() << "\n";
    return 1;
  }
}
