"""options/train_options.py of the reference (same flags and defaults), and the optimizer options beyond its recipe."""
from .base_options import BaseOptions, _bool


class TrainOptions(BaseOptions):
    def initialize(self):
        BaseOptions.initialize(self)
        p = self.parser
        p.add_argument('--lr', type=float, default=2.5e-4, help='initial learning rate')
        p.add_argument('--agent_lr', type=float, default=5.0e-5, help='initial agent learning rate')
        # torch.optim.RMSprop's other options and gradient-norm clipping (0 = off: the reference's recipe, stack-hg.py:51-52); the pose
        # net's and the agent's optimizers get the same values (utils/optim.py)
        p.add_argument('--momentum', type=float, default=0., help='RMSprop momentum (0: off)')
        p.add_argument('--weight_decay', type=float, default=0., help='RMSprop weight decay (0: off)')
        p.add_argument('--centered', type=int, default=0, help='1: centered RMSprop (0: off)')
        p.add_argument('--clip_grad_norm', type=float, default=0., help='clip the gradient to this 2-norm before the step (0: off)')
        # the optimizer itself (utils/optim.py make_optimizer; rmsprop: the reference's).  adam / adamw: torch.optim.Adam's formula,
        # --weight_decay coupled (adam) or decoupled (adamw) and passed as given, --clip_grad_norm as above; --momentum and --centered
        # are RMSprop's and refused with them
        p.add_argument('--optimizer', type=str, default='rmsprop', choices=('rmsprop', 'adam', 'adamw', 'sgd', 'lars', 'lamb'),
                       help='optimizer of the pose net and the agent')
        p.add_argument('--beta1', type=float, default=0.9, help='Adam / AdamW: decay of the first moment')
        p.add_argument('--beta2', type=float, default=0.999, help='Adam / AdamW: decay of the second moment')
        p.add_argument('--adam_eps', type=float, default=1e-8, help='Adam / AdamW: eps added to the denominator')
        p.add_argument('--amsgrad', type=int, default=0, help='1: Adam / AdamW with AMSGrad (0: off)')
        # sgd / lars / lamb (utils/optim.py SGD, LARS, LAMB): torch.optim.SGD's formula with --momentum (required > 0 with sgd: the flag's
        # default is RMSprop's 0, and a bare --optimizer sgd stays refused as it always was), --nesterov and --weight_decay; lars
        # scales every tensor's step by --trust_coef ||w|| / (||g|| + wd ||w|| + 1e-8); lamb is Adam's update (--beta1 --beta2 --adam_eps)
        # scaled per tensor by ||w|| / ||update||, capped at --max_trust.  Tensors without weight decay are not adapted unless --always_adapt
        p.add_argument('--nesterov', type=int, default=0, choices=(0, 1), help='sgd / lars: 1 = Nesterov momentum (needs --momentum)')
        p.add_argument('--trust_coef', type=float, default=1e-3, help='lars: trust coefficient')
        p.add_argument('--max_trust', type=float, default=0., help='lamb: cap of the trust ratio (0: none)')
        p.add_argument('--always_adapt', type=int, default=0, choices=(0, 1), help='lars / lamb: 1 = adapt tensors without weight decay too')
        # parameter groups (utils/optim.py make_optimizer, group_specs): all off by default, and then the optimizer has the one group it
        # always had.  --freeze and --lr_group select tensors of the POSE net by state-dict name (re.search); the agent's optimizer takes
        # --no_decay_1d only
        p.add_argument('--no_decay_1d', type=int, default=0, choices=(0, 1), help='1: no weight decay on BatchNorm weights / biases and conv / linear biases')
        p.add_argument('--freeze', type=str, default='', help='REGEX: pose-net tensors that keep their loaded values')
        p.add_argument('--lr_group', type=str, action='append', default=[], help='REGEX:MULT (repeatable): pose-net tensors trained at MULT times the learning rate')
        # coordinate loss beside the heat-map MSE (stack_hg.coord_criterion): W * mean |soft-arg-max(out, beta) - pts| per stack; 0 = off, the
        # reference's recipe and the fused step
        p.add_argument('--coord_loss', type=float, default=0., help='weight of the soft-arg-max coordinate L1 loss (0: off)')
        p.add_argument('--coord_beta', type=float, default=1., help='inverse temperature of the soft-arg-max of --coord_loss')
        # exponential moving average of the pose net's weights (utils/optim.py ModelEma): validation, the -preds.mat files and is_best
        # come from the averaged net, the checkpoint carries both; 0 = off, the reference's recipe: no twin net and no launch
        p.add_argument('--ema_decay', type=float, default=0., help='decay of the weight EMA that is validated and saved (0: off)')
        p.add_argument('--ema_warmup', type=int, default=0, choices=(0, 1), help='1: decay min(D, (1 + t) / (10 + t)) over the first updates')
        p.add_argument('--ema_buffers', type=str, default='ema', choices=('ema', 'copy'), help='BatchNorm running statistics of the EMA: averaged, or copied')
        # gradient accumulation (utils/optim.py accumulate(), accum_plan): the optimizer steps on the mean gradient of N micro-batches of
        # --bs each; 1 = off, the reference's recipe: a step per batch and no launch added
        p.add_argument('--accum_steps', type=int, default=1, help='micro-batches of --bs per optimizer step (1: off)')
        p.add_argument('--bs', type=int, default=12, help='mini-batch size')
        p.add_argument('--load_checkpoint', type=_bool, default=False, help='resume from checkpoint model')
        p.add_argument('--load_checkpoint_pose', type=_bool, default=False, help='use checkpoint model')
        p.add_argument('--load_checkpoint_asn', type=_bool, default=False, help='use checkpoint model')
        p.add_argument('--load_prefix_pose', type=str, default='', help='checkpoint name for resuming')
        p.add_argument('--load_prefix_sr', type=str, default='', help='checkpoint name for loading sr agent')
        p.add_argument('--load_prefix_occ', type=str, default='', help='checkpoint name for loading occ agent')
        p.add_argument('--load_prefix_aug', type=str, default='', help='checkpoint name')
        p.add_argument('--occ_dir', type=str, default='occ-dir', help='occlusion dir')
        p.add_argument('--sr_dir', type=str, default='sr-dir', help='sr dir')
        p.add_argument('--joint_dir', type=str, default='joint', help='model dir for joint training')
        p.add_argument('--nEpochs', type=int, default=100, help='number of total training epochs to run')
        p.add_argument('--best_pckh', type=float, default=0., help='best result until now')
        p.add_argument('--train_list', type=str, default='train_list.txt', help='train image list')
        p.add_argument('--val_list', type=str, default='val_list.txt', help='validation image list')
        p.add_argument('--print_freq', type=int, default=10, help='print log every n iterations')
        p.add_argument('--display_freq', type=int, default=10, help='display figures every n iterations')
        p.add_argument('--pose_gpu_id', type=int, default=0, help='gpu ids')
        p.add_argument('--asn_gpu_id', type=int, default=1, help='gpu ids')

    def parse(self, args=None):
        if not self.initialized:
            self.initialize()
        o = self.parser.parse_args(args)
        if o.optimizer in ('adam', 'adamw') and (o.momentum != 0 or o.centered):
            self.parser.error('--momentum and --centered are RMSprop options: not with --optimizer %s' % o.optimizer)
        if o.optimizer in ('sgd', 'lars', 'lamb') and (o.centered or o.amsgrad or (o.optimizer == 'lamb' and o.momentum != 0)):
            self.parser.error('--centered and --amsgrad (and, for lamb, --momentum) do not go with --optimizer %s' % o.optimizer)
        if o.optimizer == 'sgd' and o.momentum == 0:
            self.parser.error('--optimizer sgd needs --momentum > 0 (the default 0 is that of RMSprop; gradient descent without momentum is '
                              'utils.optim.SGD(net, lr) in code)')
        if o.nesterov and (o.optimizer not in ('sgd', 'lars') or o.momentum == 0):
            self.parser.error('--nesterov needs --optimizer sgd or lars and --momentum > 0')
        if o.coord_loss < 0 or not o.coord_beta > 0:
            self.parser.error('--coord_loss must be >= 0 and --coord_beta > 0')
        if not 0 <= o.ema_decay < 1:
            self.parser.error('--ema_decay must be in [0, 1) (0: off)')
        if o.accum_steps < 1:
            self.parser.error('--accum_steps must be >= 1 (1: off)')
        return BaseOptions.parse(self, args)
