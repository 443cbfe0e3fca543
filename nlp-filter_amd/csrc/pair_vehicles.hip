// Vehicle and multi-receiver pairs: kinematic bicycle (C4, nlp/dynamics.py:117-136),
// multi_receiver (nlp/dynamics.py:81-96) and gnss_two_receiver (:98-115) with
// mixed rows (C5 / gnss-multi-receiver.py).  The dynamic bicycle's pairs are in
// pair_autocar.hip (their own translation unit: the longest to compile).
#include "mhe_core.h"

namespace mhe {
const PairOps* pairs_vehicles(int dyn, int meas) {
  if (dyn == MHE_DYN_KINEMATIC_BICYCLE && meas == MHE_MEAS_PSEUDORANGE)
    return pair_ops<DynKinematicBicycle, MeasPseudorange<6>>();
  if (meas != MHE_MEAS_MIXED) return nullptr;
  switch (dyn) {
    case MHE_DYN_KINEMATIC_BICYCLE: return pair_ops<DynKinematicBicycle, MeasMixed<6>>();
    case MHE_DYN_MULTI_RECEIVER: return pair_ops<DynMultiReceiver, MeasMixed<8>>();
    case MHE_DYN_GNSS_TWO_RECEIVER: return pair_ops<DynGnssTwoReceiver, MeasMixed<10>>();
  }
  return nullptr;
}
}  // namespace mhe
