"""The subjects of tests/test_deploy_label_gzip_gpu.py and the labels the oracle gives them: phantom cines under the 'threshold'
weights (weights.threshold_params: compact regions) and the gamma-noise volumes of tests/test_deploy_gpu.py under its random weights
(noise labels).  The CPU tests of tests/test_device_label_gzip.py check on these labels that every phantom subject compresses
below nifti.NOISE_FRACTION and fits the encoder's buffers, and that no noise subject does -- which is what lets the GPU test demand
that all of the former take the device encoder and all of the latter fall back."""
import numpy as np

MODEL = 'FCN_sa'
AFFINE = np.diag([1.8, 1.8, 10.0, 1.0])
PIXDIM = np.array([1, 1.8, 1.8, 10.0, 0.03, 0, 0, 0], np.float32)
# phantom cines of the kind tests/test_deploy_gpu.py feeds the drop-in script (test_precision_flag_f32x3_writes_the_fp32_labels), smaller
# still (every one below 64 KiB of fixed-code output, the smallest capacity the pipeline gives the device encoder).  Different shapes of ONE
# voxel count: the deploy loop sizes its staging buffers by whichever volume a reader thread loads first, and a larger one would leave the
# pipeline for the one-subject path
SUBJECTS = [('subj00', (64, 80, 2, 5), 50), ('subj01', (80, 64, 2, 5), 51), ('subj02', (64, 100, 2, 4), 52), ('subj03', (80, 80, 2, 4), 8)]
# ... and the same cohort with a larger subject third: with one reader thread the first subject sizes the pipeline, so this one leaves it for
# the one-subject path and its host writer while the flag is on, and the pipeline goes on behind it
MIXED_SUBJECTS = SUBJECTS[:2] + [('subj02', (96, 100, 2, 5), 53)] + SUBJECTS[3:]


def volume(shape, seed):
    from ukbb_cardiac_amd.phantom import cine_phantom
    X, Y, Z, T = shape
    return np.round(cine_phantom(Z * T, X, Y, seed=seed)[..., 0].reshape(T, Z, X, Y).transpose(2, 3, 1, 0) * 1000.0).astype(np.float32)


# the sequence subjects of tests/test_deploy_gpu.py (test_two_shards_on_one_gpu_equal_single_process): the three of one size
NOISE_SUBJECTS = [('subj%02d' % i, (100 + 4 * (i % 3), 120, 3, 5), 50 + i) for i in (0, 3, 6)]


def noise_volume(shape, seed):
    return (1000.0 * np.random.default_rng(seed).gamma(2.0, 1.0, size=shape)).astype(np.float32)


def cohort(weights):
    """(subjects, volume function, parameters) of 'threshold', 'mixed' (sizes; 'threshold' weights) or 'random'."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params, threshold_params
    if weights in ('threshold', 'mixed'):
        return (SUBJECTS if weights == 'threshold' else MIXED_SUBJECTS), volume, threshold_params(MODELS[MODEL])
    return NOISE_SUBJECTS, noise_volume, synthetic_params(MODELS[MODEL], 1234)


def oracle_labels(weights='threshold'):
    """[(name, (X,Y,Z,T) uint8 labels)] through the host pipeline with the C oracle as the network."""
    from oracle import c_oracle
    from ukbb_cardiac_amd import pipeline
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import pack_flat
    arch = MODELS[MODEL]
    subjects, volume, params = cohort(weights)
    flat = pack_flat(arch, params)
    out = []
    for name, shape, seed in subjects:
        pred = pipeline.segment_sequence(volume(shape, seed), lambda b: {'pred': c_oracle.forward(arch, flat, b, want_logits=False)[2]}, 128, False)
        out.append((name, np.asarray(pred, np.uint8)))
    return out
