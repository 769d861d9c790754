// Link stub for host_tests (CPU-only): the scorers reference hip_gamma_model's alpha accessors, but
// the unit tests never construct a GPU model.  Any attempt to do so aborts: there is no CPU path.
#include <cstdlib>

#include "cafe_host.h"

namespace cafe {
void hip_gamma_model::set_alpha(double) { std::abort(); }
// branch_change_tests checks the reports' arithmetic on tables it writes down; the device call behind them has no CPU path either
branch_change_result hip_model_base::branch_change(root_equilibrium_distribution*, const std::map<int, int>&, int, double, const std::vector<const clade*>&) {
    std::abort();
}
}  // namespace cafe
