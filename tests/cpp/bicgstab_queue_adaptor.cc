// Drives Dune::HipBiCGSTABSolver::apply_queue (any number of right-hand sides through a BiCGSTAB block of fixed width,
// ddm_bicgstab_solve_queue) on the objects that queue_adaptor.cc builds, combined multiplicatively (a non-symmetric preconditioner):
// SchwarzPreconditioner (ILU(0)) + POU GalerkinPreconditioner in a CombinedPreconditioner, NonOverlappingOperator, BiCGSTAB on the
// device.  Single rank (mock communication, see mock/).  apply_queue lives in the base class of the device Krylov solvers: a solver
// without a queued loop (restarted GMRES) must throw Dune::NotImplemented.
//   usage: bicgstab_queue_adaptor <dir with rowptr.bin col.bin val.bin dirichlet.bin pou.bin rhs.bin> <M> <width>
// rhs.bin: the M right-hand sides as an n x M row-major block.  Writes the solutions to <dir>/x_queue.bin in the same layout, prints
// "col <c> <iterations> <converged> <reduction>" per column, "b_unchanged <0|1>", "errors_caught <k>" (an empty column list, width 33, GMRES) and then "queue_ok".
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
  if (argc < 4) return 2;
  const std::string dir = argv[1];
  const int m = std::atoi(argv[2]), width = std::atoi(argv[3]);
  using Vec = Dune::BlockVector<Dune::FieldVector<double, 1>>;
  using Mat = Dune::BCRSMatrix<Dune::FieldMatrix<double, 1, 1>>;
  using Comm = Dune::OwnerOverlapCopyCommunication<std::size_t, int>;
  try {
    auto rp64 = slurp<int64_t>(dir + "/rowptr.bin");
    auto ci32 = slurp<int32_t>(dir + "/col.bin");
    auto va = slurp<double>(dir + "/val.bin");
    auto dm = slurp<unsigned char>(dir + "/dirichlet.bin");
    auto pw = slurp<double>(dir + "/pou.bin");
    auto rhs = slurp<double>(dir + "/rhs.bin");
    const std::size_t n = rp64.size() - 1;
    if (m < 1 || rhs.size() != n * (std::size_t)m) { std::cerr << "rhs.bin does not hold n x M doubles\n"; return 2; }
    auto A = std::make_shared<Mat>(n, n, std::vector<std::size_t>(rp64.begin(), rp64.end()), std::vector<std::size_t>(ci32.begin(), ci32.end()), va);
    auto comm = std::make_shared<Comm>();
    for (std::size_t i = 0; i < n; ++i) comm->indexSet().v.push_back({i, {i, Dune::OwnerOverlapCopyAttributeSet::owner}});

    Dune::ParameterTree ptree;
    ptree.sub("schwarz")["type"] = "standard";
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
    Dune::HipBiCGSTABSolver<Vec> solver(op, prec, 1e-9, 200);

    std::vector<Vec> B(m, Vec(n)), X(m, Vec(n));
    for (int c = 0; c < m; ++c)
      for (std::size_t i = 0; i < n; ++i) {
        B[c][i] = rhs[i * m + c];
        X[c][i] = 0.0;
      }
    std::vector<Dune::InverseOperatorResult> res;
    solver.apply_queue(X, B, width, res);   // one upload, one queued solve, one download
    bool ok = res.size() == (std::size_t)m, same = true;
    std::vector<double> xout(n * (std::size_t)m);
    for (int c = 0; c < m; ++c) {
      for (std::size_t i = 0; i < n; ++i) {
        xout[i * m + c] = X[c][i][0];
        same = same && B[c][i][0] == rhs[i * m + c];
      }
      std::printf("col %d %d %d %.3e\n", c, res[c].iterations, res[c].converged ? 1 : 0, res[c].reduction);
      ok = ok && res[c].converged;
    }
    std::printf("b_unchanged %d\n", same ? 1 : 0);
    std::ofstream(dir + "/x_queue.bin", std::ios::binary).write(reinterpret_cast<const char*>(xout.data()), xout.size() * sizeof(double));
    int caught = 0;
    try {
      std::vector<Vec> x0, b0;
      solver.apply_queue(x0, b0, width, res);   // no column
    } catch (Dune::InvalidStateException&) { ++caught; }
    try {
      solver.apply_queue(X, B, 33, res);        // wider than a block
    } catch (Dune::InvalidStateException&) { ++caught; }
    try {
      Dune::HipRestartedGMResSolver<Vec> gmres(op, prec, 1e-9, 30, 200);
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
