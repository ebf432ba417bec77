// The key [schwarz] multi_engine = levels | xcd of SchwarzPreconditioner (dune/ddm/hip/schwarz.hh -> ddm_schwarz_set_multi_engine): the
// two-level preconditioner of examples/poisson.cc:229-321 is built twice, once per value, and Dune::HipCGSolver's block apply
// (std::vector<X> of right-hand sides) runs on each.  The engine only changes how the local solves of the block applies are launched,
// so iteration counts, reductions, solutions and final defects must agree BITWISE; ddm_ilu0_multi_info on the two local solvers says
// which engine ran.  An unknown value throws Dune::NotImplemented naming it.  Single rank (mock communication, see mock/).
//   usage: multi_engine_adaptor <dir with rowptr.bin col.bin val.bin b.bin dirichlet.bin pou.bin> <m>
// prints "engines <last engine under levels> <last engine under xcd> <decline under xcd>", per column "col <c> <iterations levels>
// <iterations xcd> <entries of x that differ> <entries of b that differ>", "errors_caught <n>", "multi_engine_ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "adaptor_fixture.hh"   // first: the adaptor headers below expect the dune-istl ones before them

#include <dune/ddm/hip/solvers.hh>

int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  const std::string dir = argv[1];
  const int m = std::atoi(argv[2]);
  if (m < 1) return 2;
  try {
    const Problem p = read_problem(dir);
    const auto bb = slurp<double>(dir + "/b.bin");
    const std::size_t n = p.n;
    struct Run {
      std::vector<Vec> X, B;
      std::vector<Dune::InverseOperatorResult> res;
      int64_t info[14];
    };
    auto solve = [&](const std::string& engine) {
      auto ptree = two_level_ptree("standard", "ilu0", "additive", "umfpack");
      ptree.sub("schwarz")["multi_engine"] = engine;
      const TwoLevel t = build_two_level(p, ptree);
      Dune::HipCGSolver<Vec> solver(t.op, t.prec, 1e-10, 500);
      Run r;
      r.B = seeded_columns(p, bb, m), r.X = zero_columns(n, m);
      solver.apply(r.X, r.B, 1e-10, r.res);
      auto ctx = t.prec->context();
      ddm_hip::check(ctx->handle(), ddm_schwarz_status(ctx->handle(), t.schwarz->handle(n)), "ddm_schwarz_status");   // (synchronises)
      int64_t count = 0;
      ddm_hip::check(ctx->handle(), ddm_ilu0_multi_info(ddm_schwarz_local_solver(t.schwarz->handle(n)), r.info, 14, &count), "ddm_ilu0_multi_info");
      return r;
    };
    const Run a = solve("levels"), b = solve("xcd");
    std::printf("engines %lld %lld %lld\n", (long long)a.info[1], (long long)b.info[1], (long long)b.info[2]);
    bool ok = a.info[0] == 0 && a.info[1] == 0 && b.info[0] == 1 && b.info[1] == 1 && b.info[2] == 0 && b.info[4] == 1 && a.res.size() == (std::size_t)m &&
              b.res.size() == (std::size_t)m;
    for (int c = 0; c < m && ok; ++c) {
      std::size_t dx = 0, db = 0;
      for (std::size_t i = 0; i < n; ++i) {
        const double xa = a.X[c][i], xb = b.X[c][i], ba = a.B[c][i], bbv = b.B[c][i];
        dx += std::memcmp(&xa, &xb, sizeof(double)) != 0;
        db += std::memcmp(&ba, &bbv, sizeof(double)) != 0;
      }
      std::printf("col %d %d %d %zu %zu\n", c, a.res[c].iterations, b.res[c].iterations, dx, db);
      ok = ok && a.res[c].converged && b.res[c].converged && a.res[c].iterations == b.res[c].iterations && a.res[c].iterations > 4 &&
           a.res[c].reduction == b.res[c].reduction && dx == 0 && db == 0;
    }
    int caught = 0;
    try {
      auto ptree = two_level_ptree("standard", "ilu0", "additive", "umfpack");
      ptree.sub("schwarz")["multi_engine"] = "pipe";
      const TwoLevel t = build_two_level(p, ptree);
    } catch (Dune::NotImplemented& e) {
      const std::string w = e.what();
      if (w.find("multi_engine") != std::string::npos && w.find("pipe") != std::string::npos) ++caught;
    }
    std::printf("errors_caught %d\n", caught);
    if (ok && caught == 1) std::printf("multi_engine_ok\n");
    return ok && caught == 1 ? 0 : 1;
  } catch (Dune::Exception& e) {
    std::cerr << "Dune exception: " << e.what() << "\n";
    return 1;
  }
}
