// Drives Dune::HipBlockGMResSolver ([solver] type = blockgmressolver) the way examples/poisson.cc:229-321 builds its solver: restricted
// SchwarzPreconditioner (ILU(0)) + POU GalerkinPreconditioner in a multiplicative CombinedPreconditioner -- a preconditioner that is
// not symmetric --, NonOverlappingOperator, the solver from getHipSolver.  Single rank (mock communication, see mock/).  The factory
// must return the class for the key; the block apply and the single-vector apply (the block of width 1) are checked BITWISE against
// ddm_bgmres_solve_multi called on the same device objects, and their iteration counts against the ones on the command line;
// apply_queue must throw Dune::NotImplemented; minressolver is still refused, the message naming blockgmressolver.
//   usage: bgmres_adaptor <dir with rowptr.bin col.bin val.bin b.bin dirichlet.bin pou.bin> <m> <iterations of the single solve> <m block iterations>
// prints "factory <0|1>", "single <iterations adaptor> <iterations C ABI> <expected> <entries of x that differ> <entries of b that differ>",
// per column "col <c> <iterations adaptor> <iterations C ABI> <expected> <x differ> <b differ>", "queue <0|1>", "errors_caught <n>", "bgmres_ok".
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
  if (argc < 3) return 2;
  const std::string dir = argv[1];
  const int m = std::atoi(argv[2]);
  if (m < 1 || argc != 3 + 1 + m) return 2;
  std::vector<int> expected;
  for (int a = 3; a < argc; ++a) expected.push_back(std::atoi(argv[a]));
  try {
    const Problem p = read_problem(dir);
    const std::size_t n = p.n;
    const auto bb = slurp<double>(dir + "/b.bin");
    auto ptree = two_level_ptree("restricted", "ilu0", "multiplicative", "umfpack");
    ptree.sub("solver")["type"] = "blockgmressolver";
    ptree.sub("solver")["maxit"] = "500";
    ptree.sub("solver")["restart"] = "6";
    ptree.sub("solver")["rank_tol"] = "1e-12";
    ptree.sub("solver")["reduction"] = "1e-10";
    const TwoLevel t = build_two_level(p, ptree);
    auto lop = std::static_pointer_cast<Dune::LinearOperator<Vec, Vec>>(t.op);
    auto lprec = std::static_pointer_cast<Dune::Preconditioner<Vec, Vec>>(t.prec);
    auto solver = std::dynamic_pointer_cast<Dune::HipBlockGMResSolver<Vec>>(Dune::getHipSolver<Vec>(lop, ptree.sub("solver"), lprec));
    std::printf("factory %d\n", solver ? 1 : 0);
    if (!solver) return 1;

    std::vector<Vec> B = seeded_columns(p, bb, m), X = zero_columns(n, m);
    const std::vector<Vec> Bsave = B;
    auto ctx = t.prec->context();   // the same device objects through the C ABI
    ddm_ctx* h = ctx->handle();
    ddm_op* oh = t.op->op_handle();
    ddm_combined* ph = t.prec->handle(n);
    auto c_abi = [&](const std::vector<Vec>& cols, std::vector<double>& hx, std::vector<double>& hb, std::vector<ddm_solve_result>& rr) {
      const int w = (int)cols.size();
      hb = pack(cols);
      hx.assign(n * w, 0.0);
      rr.assign(w, ddm_solve_result{});
      ddm_hip::DeviceVector dX(ctx, n * w), dB(ctx, n * w);
      ddm_hip::check(h, ddm_memcpy_h2d(h, dX.data(), hx.data(), (int64_t)(n * w * sizeof(double))), "h2d");
      ddm_hip::check(h, ddm_memcpy_h2d(h, dB.data(), hb.data(), (int64_t)(n * w * sizeof(double))), "h2d");
      ddm_hip::check(h, ddm_bgmres_solve_multi(h, oh, ph, w, dX.data(), dB.data(), 1e-10, 500, 6, 1e-12, nullptr, nullptr, rr.data()), "ddm_bgmres_solve_multi");
      ddm_hip::check(h, ddm_memcpy_d2h(h, hx.data(), dX.data(), (int64_t)(n * w * sizeof(double))), "d2h");
      ddm_hip::check(h, ddm_memcpy_d2h(h, hb.data(), dB.data(), (int64_t)(n * w * sizeof(double))), "d2h");
    };
    auto differing = [&](const Vec& v, const std::vector<double>& a, int w, int c) {
      std::size_t d = 0;
      for (std::size_t i = 0; i < n; ++i) {
        const double x = v[i];
        d += std::memcmp(&x, &a[i * w + c], sizeof(double)) != 0;
      }
      return d;
    };
    bool ok = true;
    std::vector<double> hx, hb;
    std::vector<ddm_solve_result> rr;
    {
      Vec x1(n), b1 = Bsave[0];
      x1 = 0;
      Dune::InverseOperatorResult r1;
      solver->apply(x1, b1, 1e-10, r1);   // the block of width 1
      c_abi(std::vector<Vec>(1, Bsave[0]), hx, hb, rr);
      const std::size_t dxn = differing(x1, hx, 1, 0), dbn = differing(b1, hb, 1, 0);
      std::printf("single %d %d %d %zu %zu\n", r1.iterations, rr[0].iterations, expected[0], dxn, dbn);
      ok = ok && r1.converged && rr[0].converged && r1.iterations == rr[0].iterations && r1.iterations == expected[0] && r1.iterations > 4 &&
           r1.reduction == rr[0].reduction && dxn == 0 && dbn == 0;
    }
    {
      std::vector<Dune::InverseOperatorResult> res;
      solver->apply(X, B, 1e-10, res);   // one upload, one block solve, one download
      c_abi(Bsave, hx, hb, rr);
      ok = ok && res.size() == (std::size_t)m;
      for (int c = 0; c < m && ok; ++c) {
        const std::size_t dxn = differing(X[c], hx, m, c), dbn = differing(B[c], hb, m, c);
        std::printf("col %d %d %d %d %zu %zu\n", c, res[c].iterations, rr[c].iterations, expected[1 + c], dxn, dbn);
        ok = ok && res[c].converged && rr[c].converged && res[c].iterations == rr[c].iterations && res[c].iterations == expected[1 + c] &&
             res[c].reduction == rr[c].reduction && dxn == 0 && dbn == 0;
      }
    }
    int threw = 0;
    try {   // there is no queued block GMRES
      std::vector<Vec> Bq = Bsave, Xq = zero_columns(n, m);
      std::vector<Dune::InverseOperatorResult> res;
      solver->apply_queue(Xq, Bq, 2, res);
    } catch (Dune::NotImplemented&) {
      threw = 1;
    }
    std::printf("queue %d\n", threw);
    int caught = 0;
    try {   // an unknown key still throws, now naming eight solvers
      Dune::ParameterTree other;
      other["type"] = "minressolver";
      Dune::getHipSolver<Vec>(lop, other, lprec);
    } catch (Dune::NotImplemented& e) {
      const std::string w = e.what();
      if (w.find("minressolver") != std::string::npos && w.find("blockgmressolver") != std::string::npos && w.find("blockcgsolver") != std::string::npos && w.find("bicgstabsolver") != std::string::npos) ++caught;
    }
    std::printf("errors_caught %d\n", caught);
    if (ok && threw == 1 && caught == 1) std::printf("bgmres_ok\n");
    return ok && threw == 1 && caught == 1 ? 0 : 1;
  } catch (Dune::Exception& e) {
    std::cerr << "Dune exception: " << e.what() << "\n";
    return 1;
  }
}
