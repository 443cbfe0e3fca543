// The dynamic bicycle with clock bias (autonomous-car.py:190-213, nlp/dynamics.py:148-174:
// vehicle_dynamics_and_gnss) with vehicle_pseudorange and with mixed rows.
#include "mhe_core.h"

namespace mhe {
const PairOps* pairs_autocar(int dyn, int meas) {
  if (dyn != MHE_DYN_VEHICLE_GNSS) return nullptr;
  if (meas == MHE_MEAS_VEHICLE_PSEUDORANGE) return pair_ops<DynVehicleGnss, MeasVehiclePseudorange>();
  if (meas == MHE_MEAS_MIXED) return pair_ops<DynVehicleGnss, MeasMixed<9>>();
  return nullptr;
}
}  // namespace mhe
