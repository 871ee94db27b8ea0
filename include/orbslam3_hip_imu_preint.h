/* Part of the C ABI of orbslam3_hip.h, which includes this file at its end: include that header, not this one.
 *
 * ---- IMU pre-integration on the device: states, links and prediction ----
 * IMU::Preintegrated (include/ImuTypes.h:143-251, src/ImuTypes.cc:107-307) as a flat record, ImuPreintState, and the four things the
 * reference does with one, each batched over streams or key frames in ONE launch, each with a host entry and a device-resident one:
 *
 *   imu_frame_measurements_batch   the interpolation loop of Tracking::PreintegrateIMU (src/Tracking.cc:1802-1845) on the samples
 *                                  orbe_unpack_batch_device wrote: mvImuFromLastFrame of every stream -> (acc, angVel, tstep)
 *   imu_preintegrate_batch         Initialize (:147-166) and IntegrateNewMeasurement (:177-235), which covers Reintegrate() (:168-175:
 *                                  reset with bu, then the list), MergePrevious (:237-261: reset, then the two lists concatenated) and
 *                                  the two accumulators of PreintegrateIMU (two jobs over the same measurements, one reset, one not)
 *   imu_links_batch                a state as the LibaLink every inertial solver of this library reads: the pre-integrated terms and
 *                                  the informations of EdgeInertial / EdgeGyroRW / EdgeAccRW (src/G2oTypes.cc:500-518)
 *   imu_predict_state_batch        the arithmetic of Tracking::PredictStateIMU (src/Tracking.cc:1873-1883, the same in both branches)
 *
 * Matrices are row major.  Biases have the order of LibaLink::bias0: bax bay baz bwx bwy bwz.  nga / nga_walk are the diagonals of
 * Calib::Cov / CovWalk: gyro x3, then accelerometer x3.
 *
 * imu_preintegrate_batch: job j optionally runs Initialize(bias) on states[state] (reset != 0: every member but nga / nga_walk is
 * reset, b = bu = bias, n_meas = 0), then integrates meas[first .. first + count) in order.  The state after every measurement
 * is the float state the reference keeps; inside one measurement the rotation increment's coefficients (sin d / d, (1 - cos d) / d^2,
 * (d - sin d) / d^3) and the polar factor U V^T of NormalizeRotation (:34-37) are taken in double and rounded once.  The first-order
 * branch applies where the float angle is below 1e-4 (:95-104).  C[9:15][9:15] only ever receives += nga_walk on its diagonal;
 * C[0:9][9:15] and C[9:15][0:9] are written by a reset alone (zero).  Every state has at most ONE writer per call.  A result does not
 * depend on what else the call carries: a job alone and the same job among thousands are bit-identical.
 *
 * imu_frame_measurements_batch: samples[b][0 .. n_imu[b]) are stream b's mvImuFromLastFrame (which samples belong to a frame stays
 * the caller's queue logic); times are ts / 1e9 in double (src/Socket/client.cc:141,143), their differences rounded to float as the
 * reference does (tab, tini, tend, tstep).  count_out[b] = max(n_imu[b] - 1, 0) measurements are written to meas_out[b][..].
 * The device entry writes count_out[b] = 0 for an n_imu[b] outside 0 .. imu_cap.
 *
 * imu_links_batch: link l = the LibaLink that imu_link() of orbslam3_shim_marshal.hpp builds on the host: the float members and
 * bias0 = b are copied; info9 = C[0:9][0:9] cast to double, inverted, symmetrised, eigen-decomposed, eigenvalues below 1e-12 set to
 * 0, recomposed, times info_scale; info_gyro / info_acc = the double inverses of C[9:12][9:12] / C[12:15][12:15] of walk_state
 * (-1: left zero).  A link whose inverse is not finite gets status[l] = ORBX_ERR_ARG and zero informations (the call still returns
 * ORBX_OK, and the other links are not affected): it is what imu_init_check / fiba_check refuse.
 *
 * imu_predict_state_batch: Rwb2 = Normalize(Rwb1 GetDeltaRotation(bias)), twb2 = twb1 + Vwb1 t + 0.5 t^2 g + Rwb1 GetDeltaPosition(bias),
 * Vwb2 = Vwb1 + t g + Rwb1 GetDeltaVelocity(bias) with t = dT, g = (0, 0, -9.81f) and the Get* of :283-307.
 *
 * Errors.  The host entries make every check before anything touches a device and return ORBX_ERR_ARG: a NULL pointer, a negative
 * size, an index or range out of bounds, two jobs of one call writing the same state, a measurement that is not finite or has
 * dt <= 0 (imu_preint_check is these checks of imu_preintegrate_batch alone, host only).  The device entries check the shapes on the
 * host (NULL, negative sizes) and only enqueue work on `stream`; bad CONTENTS are reported as ORBX_ERR_ARG in d_status[job] and leave
 * that job's output (its state) untouched.  The handle stays usable after any error.  A handle owns a stream and staging and serves
 * ONE call at a time. */
#ifndef ORBSLAM3_HIP_IMU_PREINT_H
#define ORBSLAM3_HIP_IMU_PREINT_H

typedef struct ImuMeasurement { float a[3], w[3], dt; } ImuMeasurement;      /* Preintegrated::integrable */
typedef struct ImuPreintState {          /* the numeric members of IMU::Preintegrated, row major */
    float dT, b[6], bu[6];               /* bias order of LibaLink::bias0: bax bay baz bwx bwy bwz */
    float nga[6], nga_walk[6];           /* diagonals of Calib::Cov / CovWalk: gyro x3, acc x3 */
    float dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], avgA[3], avgW[3];
    float C[225];
    int32_t n_meas;                      /* measurements integrated since the last Initialize */
} ImuPreintState;
typedef struct ImuPreintJob { int32_t state, first, count; uint8_t reset; float bias[6]; } ImuPreintJob;
typedef struct ImuLinkSpec { int32_t state, walk_state /* -1: leave zero */, kf1, kf2; double info_scale; uint8_t robust; } ImuLinkSpec;
typedef struct ImuPredictJob { int32_t state; float Rwb1[9], twb1[3], Vwb1[3], bias[6]; } ImuPredictJob;
typedef struct ImuPredictOut { float Rwb2[9], twb2[3], Vwb2[3]; } ImuPredictOut;

typedef struct imu_preint imu_preint;
int  imu_preint_create(int device, imu_preint** out);
void imu_preint_destroy(imu_preint* h);
int  imu_preint_check(const ImuPreintState* states, int n_states, const ImuPreintJob* jobs, int n_jobs, const ImuMeasurement* meas,
                      int n_meas);                                                            /* host only */
double imu_preint_last_device_ms(const imu_preint* h);      /* HIP-event time of the last host entry's launch, milliseconds */

int  imu_preintegrate_batch(imu_preint* h, ImuPreintState* states, int n_states, const ImuPreintJob* jobs, int n_jobs,
                            const ImuMeasurement* meas, int n_meas, int32_t* status /* [n_jobs] */);
int  imu_preintegrate_batch_device(imu_preint* h, ImuPreintState* d_states, int n_states, const ImuPreintJob* d_jobs, int n_jobs,
                                   const ImuMeasurement* d_meas, int n_meas, int32_t* d_status, void* stream);

int  imu_frame_measurements_batch(imu_preint* h, const OrbeImuSample* samples /* [batch][imu_cap] */, const int32_t* n_imu,
                                  const int64_t* t_prev_ns, const int64_t* t_cur_ns, int batch, int imu_cap,
                                  ImuMeasurement* meas_out /* [batch][imu_cap] */, int32_t* count_out);
int  imu_frame_measurements_batch_device(imu_preint* h, const OrbeImuSample* d_samples, const int32_t* d_n_imu, const int64_t* d_t_prev_ns,
                                         const int64_t* d_t_cur_ns, int batch, int imu_cap, ImuMeasurement* d_meas_out,
                                         int32_t* d_count_out, void* stream);

int  imu_links_batch(imu_preint* h, const ImuPreintState* states, int n_states, const ImuLinkSpec* specs, int n_links,
                     LibaLink* links_out, int32_t* status /* [n_links] */);
int  imu_links_batch_device(imu_preint* h, const ImuPreintState* d_states, int n_states, const ImuLinkSpec* d_specs, int n_links,
                            LibaLink* d_links_out, int32_t* d_status, void* stream);

int  imu_predict_state_batch(imu_preint* h, const ImuPreintState* states, int n_states, const ImuPredictJob* jobs, int n_jobs,
                             ImuPredictOut* out, int32_t* status /* [n_jobs] */);
int  imu_predict_state_batch_device(imu_preint* h, const ImuPreintState* d_states, int n_states, const ImuPredictJob* d_jobs, int n_jobs,
                                    ImuPredictOut* d_out, int32_t* d_status, void* stream);

#endif /* ORBSLAM3_HIP_IMU_PREINT_H */
