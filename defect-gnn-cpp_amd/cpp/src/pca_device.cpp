// PCA::fit_device: the data pass of PCA::fit (column means, centred scatter; reference
// pca.cpp:20-21) on the GPU through dgn_host_pca_accumulate, then PCA::fit_moments. Kept apart from
// pca.cpp, whose host-only code builds without the runtime context.
#include <stdexcept>
#include <vector>

#include "dgn/runtime.hpp"
#include "topology/betti_features.hpp"
#include "topology/pca.hpp"

namespace defect_gnn::topology {

void PCA::fit_device(const dgn::MatrixXd& x, int n_components) {
    if (x.cols() != BETTI_FEATURE_DIM)
        throw std::runtime_error("Inputted Matrix does not have the correct number of columns");  // pca.cpp:16-18
    if (n_components < 0 || n_components > BETTI_FEATURE_DIM) throw std::invalid_argument("PCA: bad n_components");
    // the C ABI takes rows contiguous; MatrixXd is column-major
    std::vector<double> rows(static_cast<size_t>(x.size()));
    for (std::ptrdiff_t i = 0; i < x.rows(); ++i)
        for (std::ptrdiff_t k = 0; k < x.cols(); ++k) rows[static_cast<size_t>(i * x.cols() + k)] = x(i, k);
    dgn_pca_moments m;
    dgn_pca_moments_init(&m);
    auto& rt = dgn::runtime();
    {
        std::lock_guard<std::mutex> lk(rt.mu);
        dgn::check(dgn_host_pca_accumulate(rt.ctx, rows.data(), x.rows(), &m), "PCA::fit_device");
    }
    fit_moments(m, n_components);
}

}  // namespace defect_gnn::topology
