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
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include <dune/istl/bcrsmatrix.hh>
#include <dune/istl/bvector.hh>
#include <dune/istl/owneroverlapcopy.hh>

#include <dune/ddm/hip/combined_preconditioner.hh>
#include <dune/ddm/hip/galerkin_preconditioner.hh>
#include <dune/ddm/hip/nonoverlapping_operator.hh>
#include <dune/ddm/hip/schwarz.hh>
#include <dune/ddm/hip/coarse_spaces.hh>
#include <dune/ddm/hip/solvers.hh>

template <class T>
static std::vector<T> slurp(const std::string& f)
{
  std::ifstream in(f, std::ios::binary | std::ios::ate);
  if (!in) { std::cerr << "cannot open " << f << "\n"; std::exit(2); }
  const std::size_t bytes = in.tellg();
  in.seekg(0);
  std::vector<T> v(bytes / sizeof(T));
  in.read(reinterpret_cast<char*>(v.data()), bytes);
  return v;
}

int main(int argc, char** argv)
{
  if (argc < 3) return 2;
  const std::string dir = argv[1];
  const int m = std::atoi(argv[2]);
  using Vec = Dune::BlockVector<Dune::FieldVector<double, 1>>;
  using Mat = Dune::BCRSMatrix<Dune::FieldMatrix<double, 1, 1>>;
  using Comm = Dune::OwnerOverlapCopyCommunication<std::size_t, int>;
  try {
    auto rp64 = slurp<int64_t>(dir + "/rowptr.bin");
    auto ci32 = slurp<int32_t>(dir + "/col.bin");
    auto va = slurp<double>(dir + "/val.bin");
    auto bb = slurp<double>(dir + "/b.bin");
    auto dm = slurp<unsigned char>(dir + "/dirichlet.bin");
    auto pw = slurp<double>(dir + "/pou.bin");
    const std::size_t n = rp64.size() - 1;
    auto A = std::make_shared<Mat>(n, n, std::vector<std::size_t>(rp64.begin(), rp64.end()), std::vector<std::size_t>(ci32.begin(), ci32.end()), va);
    auto comm = std::make_shared<Comm>();
    for (std::size_t i = 0; i < n; ++i) comm->indexSet().v.push_back({i, {i, Dune::OwnerOverlapCopyAttributeSet::owner}});

    Dune::ParameterTree ptree;
    ptree.sub("schwarz")["type"] = "restricted";
    ptree.sub("schwarz").sub("subdomain_solver")["type"] = "ilu0";
    ptree.sub("combined_preconditioner")["mode"] = "multiplicative";
    ptree.sub("coarse_solver")["type"] = "umfpack";
    auto pou = std::make_shared<PartitionOfUnity>(pw);
    auto schwarz = std::make_shared<SchwarzPreconditioner<Mat, Vec, Comm>>(A, comm, pou, ptree);
    tf::Taskflow taskflow("Main taskflow");
    auto coarse_space = std::make_unique<POUCoarseSpace<Vec>>(pou, taskflow);
    std::shared_ptr<GalerkinPreconditioner<Vec, Comm>> coarse;
    auto task = taskflow.emplace([&]() {
      auto basis = coarse_space->get_basis();
      for (auto& v : basis)
        for (std::size_t i = 0; i < n; ++i)
          if (dm[i]) v[i] = 0.0;   // zero_at_dirichlet (poisson.cc:235-238)
      coarse = std::make_shared<GalerkinPreconditioner<Vec, Comm>>(*A, basis, comm, ptree, "coarse_solver");
    });
    task.name("Build coarse preconditioner").succeed(coarse_space->get_setup_task());
    tf::Executor executor(1);
    executor.run(taskflow).get();
    auto op = std::make_shared<NonOverlappingOperator<Mat, Vec, Vec, Comm>>(A, comm);
    auto prec = std::make_shared<CombinedPreconditioner<Vec>>(ptree);
    prec->set_op(op);
    prec->add(schwarz);
    prec->add(coarse);
    Dune::HipRestartedGMResSolver<Vec> solver(op, prec, 1e-10, 8, 500);

    // right-hand sides: the problem's, then seeded pseudo-random ones (zero on the Dirichlet rows like the problem's)
    std::vector<Vec> B(m, Vec(n)), X(m, Vec(n));
    unsigned long long s = 12345;
    for (int c = 0; c < m; ++c)
      for (std::size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        const double r = (double)(s >> 11) / 9007199254740992.0 - 0.5;
        B[c][i] = c == 0 ? bb[i] : (dm[i] ? 0.0 : r);
        X[c][i] = 0.0;
      }
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
      Dune::HipBiCGSTABSolver<Vec> bicg(op, prec, 1e-10, 500);
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
