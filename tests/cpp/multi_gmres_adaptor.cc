// Drives Dune::HipRestartedGMResSolver's block apply (several right-hand sides at once, ddm_gmres_solve_multi) the way
// examples/poisson.cc:229-321 builds the solver with the shipped poisson.ini: restricted SchwarzPreconditioner (ILU(0)) + POU
// GalerkinPreconditioner in a multiplicative CombinedPreconditioner, NonOverlappingOperator, GMRES(8) on the device, so that the solves
// restart.  Single rank (mock communication, see mock/).  The block solve is checked against one device solve per column; the block
// apply of a solver without a block loop (HipBiCGSTABSolver) must throw Dune::NotImplemented.
//   usage: multi_gmres_adaptor <dir with rowptr.bin col.bin val.bin b.bin dirichlet.bin pou.bin> <m>
// prints "col <c> <iterations block> <iterations single> <max |x_block - x_single|> <max |x_single|> <max |b_block - b_single|>" per
// column, then "block_ok".
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
    const auto ptree = two_level_ptree("restricted", "ilu0", "multiplicative", "umfpack");
    const TwoLevel t = build_two_level(p, ptree);
    Dune::HipRestartedGMResSolver<Vec> solver(t.op, t.prec, 1e-10, 8, 500);

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
      double diff = 0.0, mx = 0.0, bdiff = 0.0, bmx = 0.0;
      for (std::size_t i = 0; i < n; ++i) {
        diff = std::max(diff, std::fabs(X[c][i] - x1[i]));
        mx = std::max(mx, std::fabs(x1[i]));
        bdiff = std::max(bdiff, std::fabs(B[c][i] - b1[i]));   // b receives what the solver left there
        bmx = std::max(bmx, std::fabs(Bsave[c][i]));
      }
      std::printf("col %d %d %d %.3e %.3e %.3e\n", c, res[c].iterations, r1.iterations, diff, mx, bdiff);
      ok = ok && res[c].converged && r1.converged && res[c].iterations == r1.iterations && diff <= 1e-8 * mx && bdiff <= 1e-8 * bmx;
    }
    int caught = 0;
    try {
      std::vector<Vec> x0, b0;
      solver.apply(x0, b0, 1e-10, res);
    } catch (Dune::InvalidStateException&) { ++caught; }
    try {
      Dune::HipBiCGSTABSolver<Vec> bicg(t.op, t.prec, 1e-10, 500);
      std::vector<Vec> xb(1, Vec(n)), bb1(1, Bsave[0]);
      xb[0] = 0;
      bicg.apply(xb, bb1, 1e-10, res);
    } catch (Dune::NotImplemented&) { ++caught; }
    std::printf("errors_caught %d\n", caught);
    if (ok && caught == 2) std::printf("block_ok\n");
    return ok && caught == 2 ? 0 : 1;
  } catch (Dune::Exception& e) {
    std::cerr << "Dune exception: " << e.what() << "\n";
    return 1;
  }
}
