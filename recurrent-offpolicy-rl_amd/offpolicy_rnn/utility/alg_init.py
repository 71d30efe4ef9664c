"""alg_name -> trainer class (reference offpolicy_rnn/utility/alg_init.py:16-47).

The full-trajectory recurrent family and the two baselines it is compared against - the memoryless
`sac_mlp_redq_ensemble_q` and the slice trainer `sac_rnn_slice` (with `rnn_slice_length > 0`) - are in scope of this build; the
remaining reference names raise NotImplementedError with an explicit message instead of silently mapping to something else."""

# `sac_rnn_slice` stays in this tuple for the flag set the reference asserts against (`rnn_slice_length == 0`, the parser's default):
# without a slice length there is no slice trainer to build, and the name raises like the other three
_OUT_OF_SCOPE = ('sac_no_train', 'sac_mlp', 'sac_mlp_redq', 'sac_rnn_slice')


def alg_init(parameter):
    from ..algorithm.sac_full_length_rnn_ensembleQ import SACFullLengthRNNEnsembleQ
    from ..algorithm.sac_full_length_rnn_redq import SACFullLengthRNNREDQ
    from ..algorithm.sac_full_length_rnn_redq_sep_optim import SACFullLengthRNNREDQ_SEP_OPTIM
    from ..algorithm.sac_full_length_rnn_ensembleQ_sep_optim import SACFullLengthRNNENSEMBLEQ_SEP_OPTIM
    from ..algorithm.td3_full_length_rnn_ensembleQ import TD3FullLengthRNNEnsembleQ
    from ..algorithm.td3_full_length_rnn_redq import TD3FullLengthRNNREDQ
    from ..algorithm.td3_full_length_rnn_redq_sep_optim import TD3FullLengthRNNREDQ_SEP_OPTIM
    from ..algorithm.sac_mlp_redq_ensemble_q import SAC_MLP_REDQ_EnsembleQ
    table = {
        'sac_mlp_redq_ensemble_q': (SAC_MLP_REDQ_EnsembleQ, 'sac'),
        'sac_rnn_full_horizon_ensembleQ': (SACFullLengthRNNEnsembleQ, 'sac'),
        'sac_rnn_full_horizon_redQ': (SACFullLengthRNNREDQ, 'sac'),
        'sac_rnn_full_horizon_redQ_sep_optim': (SACFullLengthRNNREDQ_SEP_OPTIM, 'sac'),
        'sac_rnn_full_horizon_ensemble_q_sep_optim': (SACFullLengthRNNENSEMBLEQ_SEP_OPTIM, 'sac'),
        'td3_rnn_full_horizon_ensembleQ': (TD3FullLengthRNNEnsembleQ, 'td3'),
        'td3_rnn_full_horizon_redQ': (TD3FullLengthRNNREDQ, 'td3'),
        'td3_rnn_full_horizon_redQ_sep_optim': (TD3FullLengthRNNREDQ_SEP_OPTIM, 'td3'),
    }
    name = parameter.alg_name
    if name == 'sac_rnn_slice' and parameter.rnn_slice_length > 0:
        from ..algorithm.sac_rnn_slice import SACRNNSlice
        return SACRNNSlice(parameter)
    if name in table:
        cls, base = table[name]
        if base == 'td3':
            parameter.base_algorithm = 'td3'
        return cls(parameter)
    if name in _OUT_OF_SCOPE:
        raise NotImplementedError(f'Algorithm {name} is a transition-level / slice trainer of the reference that this build does not '
                                  f'implement; its memoryless baseline is sac_mlp_redq_ensemble_q (one efc-<E> ensemble critic).')
    raise NotImplementedError(f'Algorithm {name} has not been implemented!')
