// Drives Dune::HipBiCGSTABSolver::apply_queue (any number of right-hand sides through a BiCGSTAB block of fixed width,
// ddm_bicgstab_solve_queue) on the two-level solver of adaptor_fixture.hh, combined multiplicatively (a non-symmetric preconditioner):
// SchwarzPreconditioner (ILU(0)) + POU GalerkinPreconditioner in a CombinedPreconditioner, NonOverlappingOperator, BiCGSTAB on the
// device.  Single rank (mock communication, see mock/).  apply_queue lives in the base class of the device Krylov solvers: a solver
// without a queued loop (restarted GMRES) must throw Dune::NotImplemented.
//   usage: bicgstab_queue_adaptor <dir with rowptr.bin col.bin val.bin dirichlet.bin pou.bin rhs.bin> <M> <width>
// rhs.bin: the M right-hand sides as an n x M row-major block.  Writes the solutions to <dir>/x_queue.bin in the same layout, prints
// "col <c> <iterations> <converged> <reduction>" per column, "b_unchanged <0|1>", "errors_caught <k>" (an empty column list, width 33, GMRES) and then "queue_ok".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "adaptor_fixture.hh"   // first: the adaptor headers below expect the dune-istl ones before them

#include <dune/ddm/hip/solvers.hh>

int main(int argc, char** argv)
{
  if (argc < 4) return 2;
  const std::string dir = argv[1];
  const int m = std::atoi(argv[2]), width = std::atoi(argv[3]);
  try {
    const Problem p = read_problem(dir);
    const auto rhs = slurp<double>(dir + "/rhs.bin");
    const std::size_t n = p.n;
    if (m < 1 || rhs.size() != n * (std::size_t)m) { std::cerr << "rhs.bin does not hold n x M doubles\n"; return 2; }
    const auto ptree = two_level_ptree("standard", "ilu0", "multiplicative", "umfpack");
    const TwoLevel t = build_two_level(p, ptree);
    Dune::HipBiCGSTABSolver<Vec> solver(t.op, t.prec, 1e-9, 200);

    std::vector<Vec> B = unpack(rhs, n, m), X = zero_columns(n, m);
    std::vector<Dune::InverseOperatorResult> res;
    solver.apply_queue(X, B, width, res);   // one upload, one queued solve, one download
    bool ok = res.size() == (std::size_t)m;
    const bool same = pack(B) == rhs;
    for (int c = 0; c < m; ++c) {
      std::printf("col %d %d %d %.3e\n", c, res[c].iterations, res[c].converged ? 1 : 0, res[c].reduction);
      ok = ok && res[c].converged;
    }
    std::printf("b_unchanged %d\n", same ? 1 : 0);
    write_bin(dir + "/x_queue.bin", pack(X));
    int caught = 0;
    try {
      std::vector<Vec> x0, b0;
      solver.apply_queue(x0, b0, width, res);   // no column
    } catch (Dune::InvalidStateException&) { ++caught; }
    try {
      solver.apply_queue(X, B, 33, res);        // wider than a block
    } catch (Dune::InvalidStateException&) { ++caught; }
    try {
      Dune::HipRestartedGMResSolver<Vec> gmres(t.op, t.prec, 1e-9, 30, 200);
      gmres.apply_queue(X, B, width, res);      // restart cycles are aligned: no queued loop
    } catch (Dune::NotImplemented&) { ++caught; }
    std::printf("errors_caught %d\n", caught);
    ok = ok && same && caught == 3;
    if (ok) std::printf("queue_ok\n");
    return ok ? 0 : 1;
  } catch (Dune::Exception& e) {
    std::cerr << "Dune exception: " << e.what() << "\n";
    return 1;
  }
}
